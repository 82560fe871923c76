"""The TSDF distance field on the device (include/viso_hip.h, "TSDF distance field": viso_tsdf_distance_field; the kernels of
libviso_amd/csrc/tsdf_field.hip) against its numpy restatement (tests/field_ref.py), byte for byte on sq, state and n_sites: on a
fused map, on random tables, on lines of the longest box and at the edges of the rule.

Input condition of the test on the fused map: the restatement itself reports n_out_of_range == 0 and n_dropped == 0 (asserted
first)."""
import ctypes as C
import functools

import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import VoxelBox

import field_ref as F
import gray_ref as G
import tsdf_ref as R
import tsdf_tables as TT
from test_gpu_tsdf import POSE, _mixed_map, _param

pytestmark = pytest.mark.gpu

BIAS = 1 << 20


def _check(tsdf, entries, min_weight, box, flags=0, want=None):
    """The device's field of the box against the restatement's (`want`: already computed).  Returns the restatement's."""
    want = F.field(entries, min_weight, box, flags) if want is None else want
    f = tsdf.distance_field(box, min_weight=min_weight, unknown_is_site=bool(flags))
    sq, st, n = want
    assert f.sq.dtype == np.uint32 and f.state.dtype == np.uint8 and f.sq.shape == f.state.shape == sq.shape
    assert f.n_sites == n, (f.n_sites, n)
    assert f.state.tobytes() == st.tobytes(), np.argwhere(f.state != st)[:5]
    assert f.sq.tobytes() == sq.tobytes(), np.argwhere(f.sq != sq)[:5]
    return want


def _table(entries, log2=12, gray=False):
    tsdf = libviso_amd.TsdfMap(None, gray=gray, voxel=0.2, capacity_log2=log2)
    tsdf.add_entries(G.with_gray(entries, entries["weight"].astype(np.uint64) * 7) if gray else entries)
    return tsdf


def _entries(rows):
    """[(k, weight, sum)] as a TSDF entry array sorted by key."""
    e = np.zeros(len(rows), R.ENTRY)
    for i, (k, w, s) in enumerate(rows):
        e["k"][i], e["weight"][i], e["sum"][i] = k, w, s
    return e[np.argsort(R.keys_of(e["k"]))]


# ---- a fused map -------------------------------------------------------------------------------------------------------------------
# Placed with the restatement, at the position of a (37, 21, 70) box that holds the most voxels of the two frames (12.8 %): min_weight 1,
# since at 2 no position of the box reaches a tenth.  Axis 2 is 70 cells: a line crosses a wave's 64-lane boundary.
FUSED_LO, FUSED_SHAPE, FUSED_MIN_WEIGHT = (-70, -28, 46), (37, 21, 70), 1
FUSED_BOX = (FUSED_LO, tuple(a + b for a, b in zip(FUSED_LO, FUSED_SHAPE)))


def _fused_frames():
    rng = np.random.default_rng(4)
    d1, d2 = _mixed_map(rng, 37, 333), _mixed_map(rng, 37, 333)
    i1, i2 = (rng.integers(0, 256, (37, 333)).astype(np.uint8) for _ in range(2))
    pose2 = POSE.copy()
    pose2[:3, 3] += [0.3, 0.0, 0.4]
    return (d1, i1, POSE), (d2, i2, pose2)


def _partners_outside_only(entries, min_weight, box):
    """The number of surface voxels of the box none of whose crossing partners is inside it."""
    lo, n = F.shape_of(box)
    hi = lo + np.asarray(n)
    c = R.crossings(entries, min_weight)
    a = c["k"].astype(np.int64)
    b = a.copy()
    b[np.arange(len(c)), c["axis"]] += 1
    in_a, in_b = ((a >= lo) & (a < hi)).all(axis=1), ((b >= lo) & (b < hi)).all(axis=1)
    inside, outside = set(), set()
    for ka, kb, ia, ib in zip(map(tuple, a), map(tuple, b), in_a, in_b):
        if ia:
            (inside if ib else outside).add(ka)
        if ib:
            (inside if ia else outside).add(kb)
    return len(outside - inside)


@functools.lru_cache(maxsize=None)
def _fused_reference():
    """(entries, {flags: (sq, state, n_sites)}) of the restatement alone, with what the test needs of them asserted."""
    f1, f2 = _fused_frames()
    e, st = R.fuse([(f1[0], f1[2]), (f2[0], f2[2])], _param(), 0.2, 3, 16, 21)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0, st
    want = {flags: F.field(e, FUSED_MIN_WEIGHT, FUSED_BOX, flags) for flags in (0, F.UNKNOWN_IS_SITE)}
    sq, state, n = want[0]
    assert n >= 50, n
    assert (state == 0).mean() >= 0.1 and (state != 0).mean() >= 0.1, (state == 0).mean()
    assert _partners_outside_only(e, FUSED_MIN_WEIGHT, FUSED_BOX) >= 1
    assert want[1][2] == n + int((state == 0).sum()) and int(sq.max()) > 100 and sq.max() != F.NONE
    for v in want.values():
        for a in v[:2]:
            a.setflags(write=False)
    return e, want


@pytest.mark.parametrize("flags", (0, F.UNKNOWN_IS_SITE))
@pytest.mark.parametrize("gray", (False, True), ids=("plain", "gray"))
def test_fused_map_against_the_restatement(viso, gray, flags):
    e, want = _fused_reference()
    tsdf = libviso_amd.TsdfMap(None, gray=gray, voxel=0.2, capacity_log2=21)
    for d, img, pose in _fused_frames():
        if gray:
            tsdf.fuse(d, _param(), pose=pose, image=img)
        else:
            tsdf.fuse(d, _param(), pose=pose)
    assert tsdf.entries().tobytes() == e.tobytes()
    _check(tsdf, e, FUSED_MIN_WEIGHT, FUSED_BOX, flags, want[flags])
    if not flags:
        _check(tsdf, e, 2, FUSED_BOX)         # fewer usable voxels, other crossings
    tsdf.close()


# ---- random tables -----------------------------------------------------------------------------------------------------------------
BLOCK_N, BLOCK_ORIGIN = 24, (-7, 3, -11)
BLOCK_BOX = ([-7 - 4, 3 - 2, -11 - 20], [-7 - 4 + 33, 3 - 2 + 29, -11 - 20 + 67])      # (33, 29, 67): over the block on every side


@pytest.mark.parametrize("min_weight", (1, 3))
@pytest.mark.parametrize("seed", (0, 1, 2))
@pytest.mark.parametrize("occupancy", (0.7, 0.1, 0.01))
def test_random_tables(viso, occupancy, seed, min_weight):
    e = TT.random_block(np.random.default_rng(100 + seed), n=BLOCK_N, origin=BLOCK_ORIGIN, occupancy=occupancy)
    tsdf = _table(e, log2=15)
    sq, st, n = _check(tsdf, e, min_weight, BLOCK_BOX)
    assert n > 0 or occupancy < 0.05
    if min_weight == 3:
        # a voxel of weight 2 is unknown, and the crossings it was an end of are gone
        lo = np.asarray(BLOCK_BOX[0])
        k = e["k"].astype(np.int64) - lo
        light = e["weight"] < 3
        assert light.any() and not st[tuple(k[light].T)].any()
        st1 = F.states(e, 1, BLOCK_BOX)
        heavy = k[~light]
        lost = (st1[tuple(heavy.T)] & F.SURFACE != 0) & (st[tuple(heavy.T)] & F.SURFACE == 0)
        assert lost.any() or occupancy < 0.5
    if seed == 0:
        _check(tsdf, e, min_weight, BLOCK_BOX, F.UNKNOWN_IS_SITE)
    tsdf.close()


# ---- lines of the longest box ------------------------------------------------------------------------------------------------------
LINE_SITES = {"first": (0,), "last": (511,), "both_ends": (0, 511), "first_and_300": (0, 300)}


def _line(axis, cells, origin=(40, -300, 7)):
    """(entries, box): a box of 512 x 1 x 1 voxels along `axis` from `origin` whose cells `cells` are surface voxels: each in front,
    with its partner behind it one step along the next axis, outside the box."""
    side = (axis + 1) % 3
    rows = []
    for c in cells:
        k = list(origin)
        k[axis] += c
        p = list(k)
        p[side] += 1
        rows += [(tuple(k), 2, 100), (tuple(p), 2, -100)]
    hi = [o + 1 for o in origin]
    hi[axis] = origin[axis] + 512
    return _entries(rows), (list(origin), hi)


@pytest.mark.parametrize("sites", sorted(LINE_SITES))
@pytest.mark.parametrize("axis", (0, 1, 2))
def test_lines_at_the_capacity(viso, axis, sites):
    cells = LINE_SITES[sites]
    e, box = _line(axis, cells)
    tsdf = _table(e)
    sq, st, n = _check(tsdf, e, 2, box)
    i = np.arange(512, dtype=np.int64)
    want = np.min([(i - c) ** 2 for c in cells], axis=0)
    assert n == len(cells) and sq.shape[axis] == 512 and sq.size == 512 and np.array_equal(sq.reshape(-1), want)
    assert int(sq.max()) == {"first": 511 ** 2, "last": 511 ** 2, "both_ends": 255 ** 2, "first_and_300": 211 ** 2}[sites]
    if sites == "first_and_300":
        assert (want[151:] == (i[151:] - 300) ** 2).all() and (want[:151] == i[:151] ** 2).all()   # the far site wins from 151 on
    tsdf.close()


# ---- edges of the rule -------------------------------------------------------------------------------------------------------------
def test_edges_of_the_rule(viso):
    cases = []      # (name, entries, min_weight, box, (n_sites, n_sites with the unknown cells))
    # sum == 0 is in front: a crossing with a negative neighbour, none with a positive one
    e = _entries([((0, 0, 0), 1, 0), ((1, 0, 0), 1, -5), ((0, 3, 0), 1, 0), ((1, 3, 0), 1, 5)])
    cases.append(("sum 0 is front", e, 1, ([-2, -1, -1], [4, 5, 2]), (2, 2 + 6 * 6 * 3 - 4)))
    # a crossing whose ends have weights on either side of min_weight
    e = _entries([((0, 0, 0), 1, 9), ((0, 0, 1), 3, -9), ((5, 5, 5), 2, 1), ((5, 4, 5), 2, -1)])
    cases.append(("weights on either side", e, 2, ([-1, -1, -1], [7, 7, 7]), (2, 2 + 8 * 8 * 8 - 3)))
    cases.append(("the same at min_weight 1", e, 1, ([-1, -1, -1], [7, 7, 7]), (4, 4 + 8 * 8 * 8 - 4)))
    # a site outside the box is ignored: both ends of a crossing next to the box's face, a site of the box further away
    e = _entries([((-1, 2, 2), 1, 4), ((-2, 2, 2), 1, -4), ((9, 2, 2), 1, 4), ((9, 2, 3), 1, -4)])
    cases.append(("a site outside the box", e, 1, ([0, 0, 0], [10, 5, 5]), (2, 250 - 2 + 2)))
    # no site
    cases.append(("no site", e, 1, ([0, 0, 0], [9, 5, 5]), (0, 225)))
    cases.append(("no site, no voxel", e[:0], 1, ([3, 3, 3], [5, 70, 4]), (0, 134)))
    # one cell: a site, a usable voxel that is none, an unknown one
    cases.append(("one cell, a site", e, 1, ([9, 2, 3], [10, 3, 4]), (1, 1)))
    cases.append(("one cell, unknown", e, 1, ([8, 2, 3], [9, 3, 4]), (0, 1)))
    e1 = _entries([((9, 2, 3), 1, -4)])
    cases.append(("one cell, usable", e1, 1, ([9, 2, 3], [10, 3, 4]), (0, 0)))
    # the end of the key range: the entry at 2^20 - 1 has no upper neighbour, the cells beyond are unknown, and the entry at -2^20
    # does not appear at 2^20
    e = _entries([((BIAS - 1, 0, 0), 1, 5), ((-BIAS, 0, 0), 1, -5), ((BIAS - 2, 0, 0), 1, 5), ((0, BIAS - 1, -BIAS), 1, -1),
                  ((0, BIAS - 1, -BIAS + 1), 1, 1)])
    cases.append(("the last index of axis 0", e, 1, ([BIAS - 3, -1, -1], [BIAS + 3, 2, 2]), (0, 6 * 3 * 3 - 2)))
    cases.append(("the first index of axis 0", e, 1, ([-BIAS - 2, 0, 0], [-BIAS + 2, 1, 1]), (0, 3)))
    cases.append(("the corner of axes 1 and 2", e, 1, ([-1, BIAS - 2, -BIAS - 2], [2, BIAS + 2, -BIAS + 3]), (2, 2 + 3 * 4 * 5 - 2)))
    # the first box of int32
    lo = -(1 << 31)
    cases.append(("lo = -2^31", e, 1, ([lo, lo, lo], [lo + 3, lo + 2, lo + 65]), (0, 390)))
    cases.append(("hi = 2^31 - 1", e, 1, ([-lo - 4, -lo - 2, -lo - 66], [-lo - 1, -lo - 1, -lo - 1]), (0, 195)))
    tables = {}
    for name, e, mw, box, n_want in cases:
        key = e.tobytes()
        if key not in tables:
            tables[key] = _table(e)
        for flags, n in zip((0, F.UNKNOWN_IS_SITE), n_want):
            got = _check(tables[key], e, mw, box, flags)
            assert got[2] == n, (name, flags, got[2], n)
            if n == 0:
                assert (got[0] == F.NONE).all(), name
    for t in tables.values():
        t.close()


# ---- the call reads only -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gray", (False, True), ids=("plain", "gray"))
def test_the_map_is_untouched(viso, gray):
    e = TT.random_block(np.random.default_rng(9))
    tsdf = _table(e, log2=10, gray=gray)
    before, st = tsdf.entries(gray=gray).tobytes(), tsdf.stats()
    for _ in range(3):
        for flags in (0, F.UNKNOWN_IS_SITE):
            for mw in (1, 2):
                _check(tsdf, e, mw, ([-6, -6, -6], [7, 7, 7]), flags)
    assert tsdf.entries(gray=gray).tobytes() == before and tsdf.stats() == st
    for mw in (1, 2, 3):
        assert tsdf.surface(mw).tobytes() == R.crossings(e, mw).tobytes()
    tsdf.close()


# ---- refusals behind a live handle ---------------------------------------------------------------------------------------------------
def test_refusals_behind_a_live_handle(viso):
    L = viso
    e = TT.random_block(np.random.default_rng(9))
    tsdf = _table(e, log2=10)
    box = VoxelBox((C.c_int32 * 3)(-4, -4, -4), (C.c_int32 * 3)(0, 1, 2))     # 4 x 5 x 6 cells
    sq, st, n = np.full(120, 77, np.uint32), np.full(120, 77, np.uint8), C.c_size_t(99)
    args = (C.byref(box), 0, sq.ctypes.data_as(C.POINTER(C.c_uint32)), st.ctypes.data_as(C.POINTER(C.c_uint8)))
    # n_cap one short: nothing written
    assert L.viso_tsdf_distance_field(tsdf.h, 1, *args, 119, C.byref(n)) == -1
    assert b"viso_tsdf_distance_field" in L.viso_last_error() and (sq == 77).all() and (st == 77).all() and n.value == 99
    # exactly enough; without a state and without a count
    assert L.viso_tsdf_distance_field(tsdf.h, 1, *args, 120, C.byref(n)) == 1
    want = F.field(e, 1, ([-4, -4, -4], [0, 1, 2]))
    assert sq.tobytes() == want[0].tobytes() and st.tobytes() == want[1].tobytes() and n.value == want[2] > 0
    sq[:] = 77
    assert L.viso_tsdf_distance_field(tsdf.h, 1, args[0], 0, args[2], None, 120, None) == 1 and sq.tobytes() == want[0].tobytes()
    # an overflowed map refuses
    many = np.zeros(1025, R.ENTRY)
    many["k"][:, 0] = np.arange(1025) + 500
    many["weight"], many["sum"] = 1, -7
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.add_entries(many)
    sq[:] = 77
    assert L.viso_tsdf_distance_field(tsdf.h, 1, *args, 120, C.byref(n)) == -4 and b"overflowed" in L.viso_last_error() and (sq == 77).all()
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.distance_field(([-4, -4, -4], [0, 1, 2]))
    tsdf.clear()
    assert tsdf.distance_field(([-4, -4, -4], [0, 1, 2]), min_weight=1).n_sites == 0
    h = tsdf.h
    tsdf.close()
    assert L.viso_tsdf_distance_field(h, 1, *args, 120, C.byref(n)) == -1 and b"not a live" in L.viso_last_error()   # a destroyed map
    # a map whose context is gone
    ctx = libviso_amd.Context(0)
    orphan = libviso_amd.TsdfMap(ctx, voxel=0.2, capacity_log2=10)
    orphan.add_entries(e)
    ctx.close()
    assert L.viso_tsdf_distance_field(orphan.h, 1, *args, 120, C.byref(n)) == -1 and b"context has been destroyed" in L.viso_last_error()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        orphan.distance_field(([-4, -4, -4], [0, 1, 2]))
    assert (sq == 77).all()
    orphan.close()
