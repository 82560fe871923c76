"""The maps' eviction (include/viso_hip.h, "Map eviction") as far as no device is needed: the restatements of tests/evict_ref.py
against the library's host-only calls and against each other, the hand-made tables that tests/test_gpu_evict.py loads, and the
argument refusals."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import MAP_ENTRY_DTYPE, TSDF_ENTRY_DTYPE, TSDF_GRAY_ENTRY_DTYPE, VoxelBox

import evict_ref as E
import gray_ref as G
import map_ref as M
import tsdf_ref as R

KINDS = ((R, TSDF_ENTRY_DTYPE), (M, MAP_ENTRY_DTYPE), (G, TSDF_GRAY_ENTRY_DTYPE))


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def test_struct_layout():
    assert C.sizeof(VoxelBox) == 24 and VoxelBox.lo.offset == 0 and VoxelBox.hi.offset == 12


def test_box_around_equals_restatement():
    rng = np.random.default_rng(1)
    cases = [(rng.uniform(-300, 300, 3), float(rng.uniform(0, 80)), float(rng.choice([0.05, 0.2, 0.5, 1.0, 3.7]))) for _ in range(300)]
    cases += [(rng.uniform(-300, -1, 3), 0.5, 0.2) for _ in range(20)]                       # negative coordinates
    cases += [(np.array([0.2 * 7, -0.2 * 3, 0.0]), 0.4, 0.2), (np.array([1.0, -2.0, 3.0]), 1.0, 0.5), (np.array([1.0, -2.0, 3.0]), 0.0, 0.5),
              (np.array([0.3, -0.3, 7.1]), 0.0, 0.2)]                                        # a centre on a voxel face; r = 0
    cases += [(np.array([1e12, -1e12, 0.0]), 1.0, 1e-3), (np.array([0.0, 0.0, 0.0]), 1e300, 1e-300),
              (np.array([429496.0, -429496.7, 0.0]), 0.3, 1e-4)]                             # clamped to int32
    for c, r, v in cases:
        lo, hi = libviso_amd.voxel_box(c, r, v)
        wlo, whi = E.box_around(c, r, v)
        assert lo.dtype == hi.dtype == np.int32 and np.array_equal(lo, wlo) and np.array_equal(hi, whi), (c, r, v, lo, hi, wlo, whi)
        assert (lo <= hi).all()
    # by hand: voxel 0.5 (exact), centre 1, r = 1: [0, 2] metres touches the voxels 0 .. 4
    lo, hi = libviso_amd.voxel_box([1.0, -2.0, 3.0], 1.0, 0.5)
    assert lo.tolist() == [0, -6, 4] and hi.tolist() == [5, -1, 9]
    lo, hi = libviso_amd.voxel_box([1.0, -2.0, 3.0], 0.0, 0.5)       # r = 0: the one voxel of the point
    assert lo.tolist() == [2, -4, 6] and hi.tolist() == [3, -3, 7]


def test_box_around_refusals():
    L = libviso_amd.load()
    b = VoxelBox()
    c = (C.c_double * 3)(1.0, 2.0, 3.0)
    assert L.viso_voxel_box_around(c, 1.0, 0.2, C.byref(b)) == 1
    for r, v in ((-1.0, 0.2), (float("nan"), 0.2), (float("inf"), 0.2), (1.0, 0.0), (1.0, -0.2), (1.0, float("nan")), (1.0, float("inf"))):
        assert L.viso_voxel_box_around(c, r, v, C.byref(b)) == -1, (r, v)
        assert b"viso_voxel_box_around" in L.viso_last_error()
    for bad in (float("nan"), float("inf")):
        assert L.viso_voxel_box_around((C.c_double * 3)(1.0, bad, 3.0), 1.0, 0.2, C.byref(b)) == -1
    assert L.viso_voxel_box_around(None, 1.0, 0.2, C.byref(b)) == -1 and L.viso_voxel_box_around(c, 1.0, 0.2, None) == -1
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        libviso_amd.voxel_box([0, 0, 0], -1.0, 0.2)


def test_split_by_hand():
    e = np.zeros(5, TSDF_ENTRY_DTYPE)
    e["k"] = [[3, 0, 0], [-1, 0, 0], [0, 0, 0], [2, 5, 0], [2, 4, -7]]
    e["weight"] = np.arange(5) + 1
    kept, gone = E.split(e, [0, 0, -7], [3, 5, 1])
    assert kept["weight"].tolist() == [3, 5] and gone["weight"].tolist() == [2, 4, 1]          # both by key: x, then y, then z
    kept, gone = E.split(e, [0, 0, 0], [0, 9, 9])                                            # an empty box
    assert len(kept) == 0 and len(gone) == 5
    kept, gone = E.split(e, [-(1 << 31)] * 3, [(1 << 31) - 1] * 3)                           # beyond +-2^20: everything on that side
    assert len(kept) == 5 and len(gone) == 0


@pytest.mark.parametrize("ref,dtype", KINDS)
def test_merge_entries_equals_the_reference_merges(ref, dtype):
    assert ref.ENTRY == dtype
    rng = np.random.default_rng(dtype.itemsize)
    parts = [E.fill(rng.integers(-5, 5, (int(n), 3)), dtype, rng) for n in (200, 1, 0, 77)]
    parts = [ref.merge(p) for p in parts]            # (voxels that are distinct within a part, as a map's entries are)
    got, want = libviso_amd.merge_entries(*parts), ref.merge(*parts)
    assert _same(got, want) and (np.diff(E.keys_of(got["k"])) > 0).all()
    assert _same(libviso_amd.merge_entries(parts[0]), parts[0])
    assert _same(libviso_amd.merge_entries(parts[2], parts[2]), parts[2])
    kept, gone = E.split(want, [-2, -9, -9], [9, 9, 3])
    assert len(kept) and len(gone) and _same(libviso_amd.merge_entries(gone, kept), want)
    with pytest.raises(ValueError):
        libviso_amd.merge_entries(parts[0], np.zeros(1, KINDS[0][1] if dtype != KINDS[0][1] else KINDS[2][1]))
    with pytest.raises(ValueError):
        libviso_amd.merge_entries()


def test_hash_restatements_agree_and_the_occupied_slots_ignore_the_order():
    rng = np.random.default_rng(3)
    k = np.unique(rng.integers(-40, 40, (900, 3)), axis=0)
    keys = E.keys_of(k)
    assert [E.map_hash(x) for x in keys[:200]] == E.map_hash_np(keys[:200]).tolist()
    assert E.map_hash(0) == 0 and E.map_hash(1) == 0x5692161d100b05e5 & 0xffffffff           # splitmix64's finaliser of 1
    a = E.probe_table(keys, 10)
    assert E.reachable(a) and (a != -1).sum() == len(keys)
    for _ in range(3):
        b = E.probe_table(rng.permutation(keys), 10)
        assert np.array_equal(a != -1, b != -1) and E.reachable(b)
        assert sorted(a[a != -1].tolist()) == sorted(b[b != -1].tolist())


def test_restated_passes_leave_a_table_that_a_fresh_insert_would_give():
    """The rebuild in Python on random tables, loads 0.3 to 0.95: every survivor is found by a probe, no key is there twice, and
    the occupied slots are those of a table that never held the evicted keys."""
    rng = np.random.default_rng(4)
    for n, frac in ((300, 0.5), (700, 0.1), (900, 0.9), (975, 0.5), (1023, 0.03), (1023, 1.0)):
        k = np.unique(rng.integers(-60, 60, (4000, 3)), axis=0)
        keys = E.keys_of(k[rng.permutation(len(k))[:n]])
        t = E.probe_table(keys, 10)
        leave = set(keys[rng.random(n) < frac].tolist())
        out = E.evict_table(t, leave)
        stay = [x for x in keys.tolist() if x not in leave]
        assert sorted(out[out != -1].tolist()) == sorted(stay) and E.reachable(out), (n, frac)
        assert np.array_equal(out != -1, E.probe_table(np.array(stay, np.int64), 10) != -1), (n, frac)


def test_hand_made_table_has_the_clusters_it_is_for():
    k, outside = E.hand_keys()
    assert np.array_equal(E.inside(k, *E.HAND_BOX), ~outside) and len(np.unique(E.keys_of(k))) == len(k)
    keys = E.keys_of(k)
    t = E.probe_table(keys, E.HAND_LOG2)
    slot = {int(key): int(np.nonzero(t == key)[0][0]) for key in keys}
    gone = sorted(slot[int(key)] for key, o in zip(keys, outside) if o)
    cl = dict(E.clusters(t))
    # one cluster wraps from slot 1023 to slot 0 and loses voxels on both sides of the wrap
    assert cl[1019] == 13 and 1019 in gone and 1022 in gone and 1 in gone and 6 in gone
    # one cluster of 20 slots loses its first, a middle and its last voxel
    assert cl[300] == 20 and {300, 309, 319} <= set(gone) and not set(gone) & (set(range(301, 319)) - {309})
    # one evicted voxel alone between two empty slots (and one that stays)
    assert cl[600] == 1 and 600 in gone and cl[700] == 1 and 700 not in gone
    assert len(cl) == 4
    # survivors behind an evicted voxel have their home before it: they must move for a probe to find them
    out = E.evict_table(t, {int(key) for key, o in zip(keys, outside) if o})
    moved = sum(1 for key in keys[~outside].tolist() if int(np.nonzero(out == key)[0][0]) != slot[key])
    assert E.reachable(out) and moved >= 20
    t2 = t.copy()
    t2[np.isin(t2, keys[outside])] = -1               # what tombstones turned empty without a rebuild would leave
    assert not E.reachable(t2)


def test_argument_errors_without_a_device():
    """No handle is live without a device: every call answers with VISO_ERR_ARG and follows no pointer, whatever else is wrong."""
    L = libviso_amd.load()
    fake = C.c_void_p(4096)
    n = C.c_size_t()
    ok = VoxelBox((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4))
    bad = VoxelBox((C.c_int32 * 3)(0, 5, 0), (C.c_int32 * 3)(4, 4, 4))                       # lo > hi
    buf = np.zeros(4, TSDF_GRAY_ENTRY_DTYPE)
    for handle in (None, fake):
        for box in (C.byref(ok), C.byref(bad), None):
            for np_ in (C.byref(n), None):
                for name in ("viso_map_evict_count", "viso_tsdf_evict_count"):
                    assert getattr(L, name)(handle, box, np_) == -1
                    assert name.encode() in L.viso_last_error()
                for name in ("viso_map_evict", "viso_tsdf_evict", "viso_tsdf_evict_gray"):
                    assert getattr(L, name)(handle, box, buf.ctypes.data, 4, np_) == -1
                    assert getattr(L, name)(handle, box, None, 0, np_) == -1
                    assert name.encode() in L.viso_last_error() and b"handle" in L.viso_last_error()
    with pytest.raises(ValueError):
        libviso_amd._box_arg("t", ([0, 0], [1, 1, 1]))
    with pytest.raises(ValueError):
        libviso_amd._box_arg("t", ([0, 0, 0.5], [1, 1, 1]))
    with pytest.raises(ValueError):
        libviso_amd._box_arg("t", ([0, 0, 0], [1, 1, 1 << 31]))


def test_tool_refuses_an_archive_without_a_window(capsys):
    from libviso_amd import fuse_map
    for args in (["--archive", "a.npy"], ["--window", "-1"], ["--window", "nan"]):
        with pytest.raises(SystemExit) as e:
            fuse_map.main(["maps", "poses.txt", "calib.txt", "out.ply"] + args)
        assert e.value.code == 2
    assert "--archive needs --window" in capsys.readouterr().err
    assert "--window" in fuse_map.__doc__ and "--archive" in fuse_map.__doc__
