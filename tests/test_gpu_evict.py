"""The maps' eviction on the device (include/viso_hip.h, "Map eviction": viso_map_evict*, viso_tsdf_evict*; the kernels of
libviso_amd/csrc/voxel_hash.h) against its numpy restatement (tests/evict_ref.py), byte for byte on the sorted entry arrays of all
three kinds of map, on fused maps, on hand-made probe clusters, on an exactly full table and over many rounds of one small table.

Input condition of the bit-exact tests on fused maps: the restatement itself reports n_out_of_range == 0 and n_dropped == 0
(asserted first).  The deliberate overflow cases are the exception."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import MAP_ENTRY_DTYPE, TSDF_ENTRY_DTYPE, TSDF_GRAY_ENTRY_DTYPE, VoxelBox

import evict_ref as E
import gray_ref as G
import map_ref as M
import mesh_ref as MR
import render_ref as RR
import tsdf_ref as R
import tsdf_tables as TT
from test_gpu_tsdf import POSE, _mixed_map, _param

pytestmark = pytest.mark.gpu

KINDS = ("tsdf", "gray", "map")
DTYPE = dict(tsdf=TSDF_ENTRY_DTYPE, gray=TSDF_GRAY_ENTRY_DTYPE, map=MAP_ENTRY_DTYPE)
MERGE = dict(tsdf=R.merge, gray=G.merge, map=M.merge)
ALL = ([-(1 << 31)] * 3, [(1 << 31) - 1] * 3)      # a box that contains every voxel
NONE = ([0, 0, 0], [5, 0, 5])                      # an empty box


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _make(kind, **params):
    if kind == "map":
        params.pop("trunc_voxels", None)
        return libviso_amd.VoxelMap(None, **params)
    return libviso_amd.TsdfMap(None, gray=kind == "gray", **params)


def _entries(kind, m):
    return m.entries(gray=True) if kind == "gray" else m.entries()


def _fuse(kind, m, d16, image, prm, pose):
    if kind == "gray":
        m.fuse(d16, prm, pose=pose, image=image)
    else:
        m.fuse(d16, prm, pose=pose)


def _ref_fuse(kind, frames, prm, voxel, min_disp16, log2):
    """frames: [(map, image, pose)].  (entries, stats) of the kind's restatement."""
    if kind == "map":
        return M.fuse([(d, p) for d, _, p in frames], prm, voxel, min_disp16, log2)
    if kind == "gray":
        return G.fuse(frames, prm, voxel, 3, min_disp16, log2)
    return R.fuse([(d, p) for d, _, p in frames], prm, voxel, 3, min_disp16, log2)


def _stats_equal(m, st, occupied):
    """The counters that the restatement has (the voxel map's n_inserts depends on the launch shape), n_occupied as given."""
    got = m.stats()
    want = dict(st, n_occupied=occupied)
    assert {k: got[k] for k in want} == want, (got, want)


@pytest.mark.parametrize("kind", KINDS)
def test_fused_map_against_the_restatement(viso, kind):
    rng = np.random.default_rng(len(kind))
    d1, d2 = _mixed_map(rng, 37, 333), _mixed_map(rng, 37, 333)
    i1, i2 = (rng.integers(0, 256, (37, 333)).astype(np.uint8) for _ in range(2))
    pose2 = POSE.copy()
    pose2[:3, 3] += [0.3, 0.0, 0.4]
    prm, voxel, log2 = _param(), 0.2, 21
    f1, f2 = (d1, i1, POSE), (d2, i2, pose2)
    want1, st1 = _ref_fuse(kind, [f1], prm, voxel, 16, log2)
    want2, st2 = _ref_fuse(kind, [f2], prm, voxel, 16, log2)
    both, st12 = _ref_fuse(kind, [f1, f2], prm, voxel, 16, log2)
    for st in (st1, st2, st12):
        assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0, st
    # a box that cuts through the data on two axes
    k = want1["k"].astype(np.int64)
    lo = [int(np.quantile(k[:, 0], 0.3)), int(k[:, 1].min()) - 3, int(k[:, 2].min()) - 3]
    hi = [int(k[:, 0].max()) + 3, int(k[:, 1].max()) + 3, int(np.quantile(k[:, 2], 0.7))]
    kept, gone = E.split(want1, lo, hi)
    assert len(kept) > 100 and len(gone) > 100
    k2 = E.keys_of(want2["k"])
    assert np.isin(k2, E.keys_of(kept["k"])).any() and np.isin(k2, E.keys_of(gone["k"])).any()   # frame 2 updates survivors, re-creates evicted
    m = _make(kind, voxel=voxel, capacity_log2=log2)
    _fuse(kind, m, *f1[:2], prm, POSE)
    assert _same(_entries(kind, m), want1)
    assert m.evict_count((lo, hi)) == len(gone) and _same(_entries(kind, m), want1)              # counting reads only
    ev = m.evict((lo, hi))
    assert ev.dtype == DTYPE[kind] and _same(ev, gone) and _same(_entries(kind, m), kept)
    assert m.evict_count((lo, hi)) == 0
    _stats_equal(m, st1, len(kept))
    _fuse(kind, m, *f2[:2], prm, pose2)
    live = _entries(kind, m)
    assert (np.diff(E.keys_of(live["k"])) > 0).all()               # a duplicate key: a survivor had become unreachable
    assert _same(live, MERGE[kind](kept, want2))
    assert _same(MERGE[kind](ev, live), both) and _same(libviso_amd.merge_entries(ev, live), both)
    _stats_equal(m, {n: st1[n] + st2[n] for n in st1}, len(live))
    m.close()


def test_readers_after_an_evict(viso):
    e = TT.random_block(np.random.default_rng(9))
    lo, hi = [-2, -100, -100], [100, 100, 3]
    kept, gone = E.split(e, lo, hi)
    assert len(kept) > 100 and len(gone) > 100
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=10)      # 500 voxels in 1024 slots: long clusters
    tsdf.add_entries(e)
    assert _same(tsdf.evict((lo, hi)), gone) and _same(tsdf.entries(), kept)
    n_tri = 0
    for mw in (1, 2, 3):
        assert _same(tsdf.surface(mw), R.crossings(kept, mw))
        (v, t), (wv, wt) = tsdf.mesh(mw), MR.mesh(kept, 0.2, mw)
        assert _same(v, wv) and _same(t, wt)
        n_tri += len(t)
    assert n_tri > 100 and len(R.crossings(kept)) < len(R.crossings(e))
    tsdf.close()
    # a render of a slab that lost the columns kx < -3
    case = TT.weights_and_means()
    s, voxel, prm, shape, pose, max_depth, mw = case
    lo, hi = [-3, -100, -100], [100, 100, 100]
    kept, gone = E.split(s, lo, hi)
    assert len(kept) and len(gone)
    tsdf = libviso_amd.TsdfMap(None, voxel=voxel, capacity_log2=10)
    tsdf.add_entries(s)
    assert tsdf.evict((lo, hi), discard=True) == len(gone)
    d, w = tsdf.render(prm, shape, pose, max_depth=max_depth, min_weight=mw, weights=True)
    wd, ww = RR.render(kept, voxel, prm, shape, pose, max_depth, mw)
    assert _same(d, wd) and _same(w, ww) and (wd != R.INVALID).any()
    assert (wd != RR.render(*case)[0]).any()                           # the columns that left are seen to have left
    tsdf.close()


@pytest.mark.parametrize("kind", KINDS)
def test_hand_built_clusters(viso, kind):
    """The table of tests/test_evict_cpu.py, entered one voxel at a time so that every voxel lies in the slot the simulation says: a
    cluster that wraps the table's end and loses voxels on both sides of the wrap, one of 20 slots that loses its first, a middle
    and its last voxel, and an evicted voxel alone between two empty slots."""
    k, outside = E.hand_keys()
    e = E.fill(k, DTYPE[kind], np.random.default_rng(7))
    m = _make(kind, voxel=0.2, capacity_log2=E.HAND_LOG2)
    for i in range(len(e)):
        m.add_entries(e[i:i + 1])
    whole = MERGE[kind](e)
    kept, gone = E.split(e, *E.HAND_BOX)
    assert _same(gone, MERGE[kind](e[outside])) and _same(_entries(kind, m), whole)
    assert m.evict_count(E.HAND_BOX) == len(gone)
    assert _same(m.evict(E.HAND_BOX), gone) and _same(_entries(kind, m), kept)
    assert m.stats()["n_occupied"] == len(kept)
    # the survivors are found (an update of a voxel that a probe misses would claim a second slot for it) and the evicted come back
    m.add_entries(kept)
    assert _same(_entries(kind, m), MERGE[kind](kept, kept)) and m.stats()["n_occupied"] == len(kept)
    m.evict(NONE, discard=True)
    m.add_entries(kept)
    m.add_entries(gone)
    assert _same(_entries(kind, m), whole) and m.stats()["n_occupied"] == len(whole)
    m.close()


@pytest.mark.parametrize("kind", KINDS)
def test_exactly_full_table(viso, kind):
    """1024 distinct voxels in 2^10 slots: no empty slot, so no cluster has a first slot."""
    rng = np.random.default_rng(11)
    g = np.stack(np.meshgrid(np.arange(16), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3) - 4
    e = MERGE[kind](E.fill(g, DTYPE[kind], rng))
    assert len(e) == 1024
    m = _make(kind, voxel=0.2, capacity_log2=10)
    m.add_entries(e)
    st = m.stats()
    assert st["n_dropped"] == 0 and st["n_occupied"] == 1024 and _same(_entries(kind, m), e)
    # a box that contains everything: nothing leaves, the map is untouched
    assert m.evict_count(ALL) == 0 and len(m.evict(ALL)) == 0 and m.evict(ALL, discard=True) == 0
    assert m.stats() == st and _same(_entries(kind, m), e)
    # half
    lo, hi = [4, -100, -100], [100, 100, 100]
    kept, gone = E.split(e, lo, hi)
    assert len(kept) == len(gone) == 512
    assert m.evict_count((lo, hi)) == 512 and _same(m.evict((lo, hi)), gone) and _same(_entries(kind, m), kept)
    assert m.stats() == dict(st, n_occupied=512)
    m.add_entries(gone)
    assert _same(_entries(kind, m), e) and m.stats()["n_occupied"] == 1024 and m.stats()["n_dropped"] == 0
    # the empty box, from the full table: everything comes back, and the map fuses again
    assert _same(m.evict(NONE), e) and len(_entries(kind, m)) == 0 and m.stats()["n_occupied"] == 0
    m.add_entries(e)
    assert m.evict(NONE, discard=True) == 1024 and len(_entries(kind, m)) == 0
    prm = _param()
    d = _mixed_map(rng, 3, 130)
    img = rng.integers(0, 256, d.shape).astype(np.uint8)
    want, fst = _ref_fuse(kind, [(d, img, None)], prm, 0.2, 16, 10)
    assert fst["n_dropped"] == 0 and fst["n_out_of_range"] == 0 and 0 < len(want) < 1024
    _fuse(kind, m, d, img, prm, None)
    assert _same(_entries(kind, m), want) and m.stats()["n_occupied"] == len(want)
    m.close()


def _block(step, dtype, rng):
    """About 2000 voxels of a 13^3 block that moves 13 voxels along x every step."""
    g = np.stack(np.meshgrid(*[np.arange(13)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) + [13 * step, -6, -6]
    return E.fill(g[rng.random(len(g)) < 0.91], dtype, rng)


@pytest.mark.parametrize("kind", KINDS)
def test_capacity_comes_back(viso, kind):
    """40 rounds of about 2000 fresh voxels into 4096 slots, the block before leaving each time: 80000 voxels pass through.  A slot
    that an eviction left unusable would fill the table within three rounds."""
    rng = np.random.default_rng(12)
    m = _make(kind, voxel=0.2, capacity_log2=12)
    total, prev = 0, None
    for step in range(40):
        b = MERGE[kind](_block(step, DTYPE[kind], rng))
        assert 1900 < len(b) < 2100
        m.add_entries(b)                                   # (VISO_ERR_NOMEM would raise)
        if prev is not None:
            box = ([13 * step, -100, -100], [13 * step + 13, 100, 100])
            if step % 2:
                assert _same(m.evict(box), prev)
            else:
                assert m.evict(box, discard=True) == len(prev)
        total += len(b)
        prev = b
        assert m.stats()["n_occupied"] == len(b)
    assert total > 4096 * 10 and _same(_entries(kind, m), prev)
    assert m.stats()["n_dropped"] == 0
    m.close()


def test_refusals_behind_a_live_handle(viso):
    L = libviso_amd.load()
    rng = np.random.default_rng(13)
    e = TT.random_block(rng)
    lo, hi = [-2, -100, -100], [100, 100, 3]
    kept, gone = E.split(e, lo, hi)
    box = VoxelBox((C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi))
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=10)
    tsdf.add_entries(e)
    st = tsdf.stats()
    # an output that is too small: the code, *n set, nothing written, nothing removed
    buf = np.zeros(len(gone), TSDF_ENTRY_DTYPE)
    for cap in (len(gone) - 1, 1, 0):
        n = C.c_size_t()
        assert L.viso_tsdf_evict(tsdf.h, C.byref(box), buf.ctypes.data, cap, C.byref(n)) == -1
        assert n.value == len(gone) and not buf["weight"].any() and b"viso_tsdf_evict" in L.viso_last_error()
        assert _same(tsdf.entries(), e) and tsdf.stats() == st
    # a box with lo > hi, a null box, a null n
    n = C.c_size_t(77)
    bad = VoxelBox((C.c_int32 * 3)(0, 5, 0), (C.c_int32 * 3)(4, 4, 4))
    for args in ((C.byref(bad), C.byref(n)), (None, C.byref(n)), (C.byref(box), None)):
        assert L.viso_tsdf_evict_count(tsdf.h, *args) == -1
        assert L.viso_tsdf_evict(tsdf.h, args[0], buf.ctypes.data, len(buf), args[1]) == -1
        assert L.viso_tsdf_evict(tsdf.h, args[0], None, 0, args[1]) == -1
    assert n.value == 77 and _same(tsdf.entries(), e) and tsdf.stats() == st
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        tsdf.evict(([0, 5, 0], [4, 4, 4]))
    # the kinds do not mix; the count takes either
    gray = libviso_amd.TsdfMap(None, gray=True, voxel=0.2, capacity_log2=10)
    ge = G.with_gray(e, rng.integers(0, 256, len(e)).astype(np.uint64) * e["weight"])
    gray.add_entries(ge)
    gbuf = np.zeros(len(gone), TSDF_GRAY_ENTRY_DTYPE)
    assert L.viso_tsdf_evict(gray.h, C.byref(box), None, 0, C.byref(n)) == -1 and b"intensity" in L.viso_last_error()
    assert L.viso_tsdf_evict(gray.h, C.byref(box), buf.ctypes.data, len(buf), C.byref(n)) == -1
    assert L.viso_tsdf_evict_gray(tsdf.h, C.byref(box), gbuf.ctypes.data, len(gbuf), C.byref(n)) == -1 and b"intensity" in L.viso_last_error()
    assert gray.evict_count((lo, hi)) == len(gone) == tsdf.evict_count((lo, hi))
    assert _same(gray.entries(gray=True), ge) and _same(tsdf.entries(), e)
    # discard returns the count; an exact capacity is enough
    assert gray.evict((lo, hi), discard=True) == len(gone) and _same(gray.entries(gray=True), E.split(ge, lo, hi)[0])
    assert L.viso_tsdf_evict(tsdf.h, C.byref(box), buf.ctypes.data, len(buf), C.byref(n)) == 1 and n.value == len(gone) and _same(buf, gone)
    gray.close()
    # an overflowed map refuses
    many = np.zeros(1025, TSDF_ENTRY_DTYPE)
    many["k"][:, 0] = np.arange(1025) + 500
    many["weight"], many["sum"] = 1, -7
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.add_entries(many)
    for call in (lambda: tsdf.evict_count((lo, hi)), lambda: tsdf.evict((lo, hi)), lambda: tsdf.evict((lo, hi), discard=True), lambda: tsdf.evict(NONE)):
        with pytest.raises(libviso_amd.VisoError, match="-4"):
            call()
    tsdf.clear()
    assert tsdf.evict(NONE, discard=True) == 0
    h = tsdf.h
    tsdf.close()
    assert L.viso_tsdf_evict_count(h, C.byref(box), C.byref(n)) == -1 and b"not a live" in L.viso_last_error()   # a destroyed map


# ---- a windowed run: a small table follows the camera and, with its archive, is the unbounded map ------------------------------------
# voxel, min_disp16 and the window's half side, chosen with the restatement: more than 1024 voxels in all (4005, 4005, 2309), never
# more than 768 live, and a window in which hundreds of voxels survive every step
WIN_LOG2, WIN_FRAMES, WIN_STEP = 10, 12, 2.0
WIN = dict(tsdf=dict(voxel=0.2, min_disp16=16 * 30, half=4.0), gray=dict(voxel=0.2, min_disp16=16 * 30, half=4.0),
           map=dict(voxel=0.02, min_disp16=16 * 20, half=5.0))


def _window_frames(rng):
    frames = []
    for i in range(WIN_FRAMES):
        d = _mixed_map(rng, 3, 130)
        pose = np.eye(4)
        pose[2, 3] = WIN_STEP * i
        frames.append((d, rng.integers(0, 256, d.shape).astype(np.uint8), pose))
    return frames


@pytest.mark.parametrize("kind", KINDS)
def test_windowed_run_equals_unbounded_run(viso, kind):
    rng = np.random.default_rng(14)
    frames = _window_frames(rng)
    prm = _param()
    voxel, md, WIN_HALF = WIN[kind]["voxel"], WIN[kind]["min_disp16"], WIN[kind]["half"]
    slots = 1 << WIN_LOG2
    whole, st = _ref_fuse(kind, frames, prm, voxel, md, 26)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0 and len(whole) > slots, len(whole)
    # the restatement of the windowed run never holds more than 3/4 of the slots
    live = np.zeros(0, DTYPE[kind])
    peak, survivors = 0, 0
    boxes = []
    for d, img, pose in frames:
        box = E.box_around(pose[:3, 3], WIN_HALF, voxel)
        boxes.append(box)
        stay = E.split(live, *box)[0]
        survivors += len(stay)
        live = MERGE[kind](stay, _ref_fuse(kind, [(d, img, pose)], prm, voxel, md, 26)[0])
        peak = max(peak, len(live))
    assert peak <= slots * 3 // 4 and survivors > 1000, (peak, survivors)
    print(f"{kind}: {len(whole)} voxels in all, at most {peak} live in {slots} slots")
    # the device: windowed at the small capacity, with an archive
    m = _make(kind, voxel=voxel, min_disp16=md, capacity_log2=WIN_LOG2)
    archive = []
    for (d, img, pose), box in zip(frames, boxes):
        dev_box = libviso_amd.voxel_box(pose[:3, 3], WIN_HALF, voxel)
        assert np.array_equal(dev_box[0], box[0]) and np.array_equal(dev_box[1], box[1])
        archive.append(m.evict(dev_box))
        _fuse(kind, m, d, img, prm, pose)
    assert sum(len(a) for a in archive) > 0
    assert _same(libviso_amd.merge_entries(*archive, _entries(kind, m)), whole)
    assert _same(_entries(kind, m), live)
    # unwindowed at the small capacity: the table fills
    m.clear()
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        for d, img, pose in frames:
            _fuse(kind, m, d, img, prm, pose)
    m.close()
