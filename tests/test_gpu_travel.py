"""The TSDF travel field on the device (include/viso_hip.h, "TSDF travel field": viso_tsdf_travel_field; the kernels of
libviso_amd/csrc/tsdf_travel.hip) against its restatement (tests/travel_ref.py: Dijkstra's algorithm with a heap), equal on cost, sq,
state, n_goals_used and n_reached: across tile seams in open space, on an empty map, through a door in a wall, along a serpentine
that re-enters tiles, on random tables, on a fused map, and at the refusals.

Input conditions, asserted on the restatement before the device is asked: the narrow door is closed and the wide one open at the
clearance used; the serpentine's far end is reached; in at least half of the random cases cells beyond the goals are reached."""
import ctypes as C
import functools

import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import VoxelBox

import field_ref as F
import travel_ref as T
import tsdf_ref as R
import tsdf_tables as TT
from test_gpu_field import BLOCK_N, BLOCK_ORIGIN, FUSED_MIN_WEIGHT, _entries, _fused_frames, _fused_reference, _table
from test_gpu_tsdf import _param
from test_travel_cpu import check_path, closed_form

pytestmark = pytest.mark.gpu

NONE = T.NONE


def _check(tsdf, want, box, flags, clearance_sq, goals, min_weight=2):
    """The device's travel field against the restatement's (cost, sq, state, n_goals_used, n_reached).  Returns the device's."""
    f = tsdf.travel_field(box, goals, clearance_sq=clearance_sq, min_weight=min_weight, unknown_is_site=bool(flags))
    cost, sq, st, used, reached = want
    assert f.cost.dtype == np.uint32 and f.field.sq.dtype == np.uint32 and f.field.state.dtype == np.uint8
    assert f.cost.shape == f.field.sq.shape == f.field.state.shape == cost.shape
    assert np.array_equal(f.field.state, st), np.argwhere(f.field.state != st)[:5]
    assert np.array_equal(f.field.sq, sq), np.argwhere(f.field.sq != sq)[:5]
    assert np.array_equal(f.cost, cost), [(tuple(c), int(f.cost[tuple(c)]), int(cost[tuple(c)])) for c in np.argwhere(f.cost != cost)[:5]]
    assert f.n_goals_used == used and f.n_reached == reached, (f.n_goals_used, used, f.n_reached, reached)
    assert f.clearance_sq == clearance_sq
    return f


def _filled(lo, shape, behind=None):
    """The entries of a box of voxels, all in front at weight 2 but for the cells of the bool mask `behind`."""
    g = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), axis=-1).reshape(-1, 3)
    e = np.zeros(len(g), R.ENTRY)
    e["k"], e["weight"], e["sum"] = g + np.asarray(lo), 2, 100
    if behind is not None:
        e["sum"][behind.reshape(-1)] = -100
    return e[np.argsort(R.keys_of(e["k"]))]


def _box(lo, shape):
    return (list(lo), [a + b for a, b in zip(lo, shape)])


# ---- tile seams in open space --------------------------------------------------------------------------------------------------------
SEAM_LO = (-5, 3, 40)


@pytest.mark.parametrize("shape", ((1, 1, 1), (7, 1, 33), (9, 8, 17), (17, 9, 8), (16, 16, 16)), ids=lambda s: "x".join(map(str, s)))
def test_tile_seams_in_open_space(viso, shape):
    e, box = _filled(SEAM_LO, shape), _box(SEAM_LO, shape)
    tsdf = _table(e, log2=14)
    far = tuple(n - 1 for n in shape)
    # the first cell, a tile's last cell, its neighbour in the next tile, the far corner: each brought into the box where it is smaller
    for goal in ((0, 0, 0), (7, 7, 7), (8, 8, 8), far):
        goal = tuple(min(g, n) for g, n in zip(goal, far))
        absolute = [[g + o for g, o in zip(goal, SEAM_LO)]]
        for flags in (0, F.UNKNOWN_IS_SITE):
            want = T.travel(e, 2, box, flags, 0, absolute)
            assert want[3] == 1 and want[4] == int(np.prod(shape)) and not (want[2] & F.SURFACE).any()
            f = _check(tsdf, want, box, flags, 0, absolute)
            assert np.array_equal(f.cost, closed_form(shape, goal)), (shape, goal)
            assert f.rounds >= 1
    tsdf.close()


# ---- an empty map --------------------------------------------------------------------------------------------------------------------
def test_empty_map(viso):
    none = _entries([])
    tsdf = _table(none)
    shape, lo = (9, 10, 19), (100, -50, -9)
    box, goal = _box(lo, shape), (4, 9, 11)
    absolute = [[g + o for g, o in zip(goal, lo)]]
    # without the flag every cell is unknown and free
    want = T.travel(none, 1, box, 0, 0, absolute)
    assert want[3] == 1 and want[4] == 9 * 10 * 19 and not want[2].any() and (want[1] == NONE).all()
    f = _check(tsdf, want, box, 0, 0, absolute, min_weight=1)
    assert np.array_equal(f.cost, closed_form(shape, goal))
    f = _check(tsdf, T.travel(none, 1, box, 0, 12345, absolute), box, 0, 12345, absolute, min_weight=1)     # NONE is at least anything
    assert np.array_equal(f.cost, closed_form(shape, goal))
    # with it every cell is a site: nothing is free, no goal is used, and the call succeeds
    want = T.travel(none, 1, box, F.UNKNOWN_IS_SITE, 0, absolute)
    assert want[3] == 0 and want[4] == 0 and (want[0] == NONE).all() and not want[1].any()
    f = _check(tsdf, want, box, F.UNKNOWN_IS_SITE, 0, absolute, min_weight=1)
    assert f.n_goals_used == 0 and f.n_reached == 0 and f.rounds == 0 and f.path(np.array(absolute[0])) is None
    tsdf.close()


# ---- a wall with a door --------------------------------------------------------------------------------------------------------------
WALL_SHAPE, WALL_LO, WALL_AT, WALL_CLEARANCE_SQ = (24, 24, 8), (-12, 30, -3), 12, 4
WALL_GOAL, WALL_FAR = (2, 12, 4), (21, 11, 3)


@functools.lru_cache(maxsize=None)
def _wall_reference(width):
    """(entries, box, goals, the restatement's field) of a wall of behind voxels across axis 0 with a door `width` cells wide."""
    behind = np.zeros(WALL_SHAPE, bool)
    behind[WALL_AT] = True
    behind[WALL_AT, 10:10 + width, :] = False
    e, box = _filled(WALL_LO, WALL_SHAPE, behind), _box(WALL_LO, WALL_SHAPE)
    goals = [[g + o for g, o in zip(WALL_GOAL, WALL_LO)]]
    want = T.travel(e, 2, box, F.UNKNOWN_IS_SITE, WALL_CLEARANCE_SQ, goals)
    for a in want[:3]:
        a.setflags(write=False)
    return e, box, goals, want


@pytest.mark.parametrize("width", (4, 5), ids=("narrow", "wide"))
def test_wall_with_a_door(viso, width):
    e, box, goals, want = _wall_reference(width)
    cost = want[0]
    # what the test needs of its input, on the restatement: the body fits through the wide door only
    assert want[3] == 1 and cost[WALL_GOAL] == 0 and (cost[:WALL_AT - 2] != NONE).all()
    assert (cost[WALL_FAR] != NONE) == (width == 5)
    assert (cost[WALL_AT + 1:] != NONE).any() == (width == 5)
    tsdf = _table(e, log2=14)
    f = _check(tsdf, want, box, F.UNKNOWN_IS_SITE, WALL_CLEARANCE_SQ, goals)
    start = np.array(WALL_FAR) + WALL_LO
    if width == 5:
        p = f.path(start)
        free = T.free_of(want[1], want[2], F.UNKNOWN_IS_SITE, WALL_CLEARANCE_SQ)
        check_path(p - np.array(WALL_LO), cost, free, WALL_FAR)
        assert (f.field.sq[tuple((p - np.array(WALL_LO)).T)] >= WALL_CLEARANCE_SQ).all()      # the way keeps its clearance
        # without a clearance the way is no longer
        wide_open = _check(tsdf, T.travel(e, 2, box, F.UNKNOWN_IS_SITE, 0, goals), box, F.UNKNOWN_IS_SITE, 0, goals)
        assert wide_open.cost[WALL_FAR] <= f.cost[WALL_FAR]
    else:
        assert f.path(start) is None
    tsdf.close()


# ---- a serpentine in voxels ----------------------------------------------------------------------------------------------------------
SERP_SHAPE, SERP_LO, SERP_WALLS, SERP_DOOR = (27, 25, 2), (7, -30, 0), range(3, 24, 4), 4


@functools.lru_cache(maxsize=None)
def _serpentine_reference():
    """Walls of behind voxels across axis 0, four cells apart (three cells of corridor: the middle one keeps sq >= 1), each open over
    SERP_DOOR cells at one end, the ends in turn: the cheapest way from the last corridor to the first one runs the length of axis 1 in
    every corridor and so re-enters every tile row."""
    behind = np.zeros(SERP_SHAPE, bool)
    for j, row in enumerate(SERP_WALLS):
        behind[row] = True
        if j % 2 == 0:
            behind[row, -SERP_DOOR:] = False
        else:
            behind[row, :SERP_DOOR] = False
    e, box = _filled(SERP_LO, SERP_SHAPE, behind), _box(SERP_LO, SERP_SHAPE)
    goals = [[o for o in SERP_LO]]
    want = T.travel(e, 2, box, F.UNKNOWN_IS_SITE, 1, goals)
    for a in want[:3]:
        a.setflags(write=False)
    return e, box, goals, want


def test_serpentine_re_enters_tiles(viso):
    e, box, goals, want = _serpentine_reference()
    cost = want[0]
    far = (26, 24, 0)      # six walls, the last one open at the low end of axis 1: the last corridor's far end is at the high end
    assert want[3] == 1 and cost[far] != NONE
    assert int(cost[far]) >= 3 * 6 * (SERP_SHAPE[1] - 2 * SERP_DOOR)          # the length of axis 1 between the doors, six times
    tsdf = _table(e, log2=14)
    f = _check(tsdf, want, box, F.UNKNOWN_IS_SITE, 1, goals)
    tiles_an_axis = max((n + 7) // 8 for n in SERP_SHAPE)
    assert f.rounds > tiles_an_axis, (f.rounds, tiles_an_axis)               # the rounds went on beyond one pass over the tiles
    p = f.path(np.array(far) + SERP_LO)
    check_path(p - np.array(SERP_LO), cost, T.free_of(want[1], want[2], F.UNKNOWN_IS_SITE, 1), far)
    tsdf.close()


# ---- random tables -------------------------------------------------------------------------------------------------------------------
RANDOM_SHAPE = (28, 27, 30)       # over the block of 24^3 on every side; 4 x 4 x 4 tiles
RANDOM_LO = (BLOCK_ORIGIN[0] - 2, BLOCK_ORIGIN[1] - 1, BLOCK_ORIGIN[2] - 3)
RANDOM_BOX = _box(RANDOM_LO, RANDOM_SHAPE)
RANDOM_CASES = [(o, s, f, c) for o in (0.7, 0.1, 0.01) for s in (0, 1, 2) for f in (0, F.UNKNOWN_IS_SITE) for c in (0, 1, 2, 9)]


@functools.lru_cache(maxsize=None)
def _random_entries(occupancy, seed):
    return TT.random_block(np.random.default_rng(100 + seed), n=BLOCK_N, origin=BLOCK_ORIGIN, occupancy=occupancy)


@functools.lru_cache(maxsize=None)
def _random_field(occupancy, seed, flags):
    want = F.field(_random_entries(occupancy, seed), 1, RANDOM_BOX, flags)
    for a in want[:2]:
        a.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def _random_reference(occupancy, seed, flags, clearance_sq):
    """(goals, the restatement's field): one to five goals, among them a cell that is not free and one outside the box wherever
    the case has such a cell; the others are free cells wherever the case has any."""
    sq, st, _ = _random_field(occupancy, seed, flags)
    free = T.free_of(sq, st, flags, clearance_sq)
    rng = np.random.default_rng([7, int(occupancy * 100), seed, flags, clearance_sq])
    cells, blocked = np.argwhere(free), np.argwhere(~free)
    n_free = min(len(cells), int(rng.integers(1, 4)))
    goals = [cells[i] for i in rng.choice(len(cells), n_free, replace=False)] if n_free else []
    if len(blocked):
        goals.append(blocked[rng.integers(len(blocked))])
    goals.append(np.array(RANDOM_SHAPE) + rng.integers(0, 3, 3) * [1, 0, 1])        # outside on axes 0 and 2
    goals = [goals[i] for i in rng.permutation(len(goals))]
    assert 1 <= len(goals) <= 5
    cost, used = T.costs(free, goals)
    assert used == n_free
    for a in (cost,):
        a.setflags(write=False)
    return (np.array(goals) + RANDOM_LO).astype(np.int32), (cost, sq, st, used, int((cost != NONE).sum()))


def test_random_cases_reach_beyond_their_goals():
    """The condition on the inputs of test_random_tables: in at least half of its cases the restatement reaches cells that are no
    goals."""
    beyond = [_random_reference(*case)[1][4] > _random_reference(*case)[1][3] for case in RANDOM_CASES]
    assert 2 * sum(beyond) >= len(RANDOM_CASES), (sum(beyond), len(RANDOM_CASES))


@pytest.mark.parametrize("occupancy,seed,flags,clearance_sq", RANDOM_CASES)
def test_random_tables(viso, occupancy, seed, flags, clearance_sq):
    goals, want = _random_reference(occupancy, seed, flags, clearance_sq)
    tsdf = _table(_random_entries(occupancy, seed), log2=15)
    _check(tsdf, want, RANDOM_BOX, flags, clearance_sq, goals, min_weight=1)
    tsdf.close()


# ---- several goals -------------------------------------------------------------------------------------------------------------------
def test_several_goals_are_the_minimum_of_each(viso):
    occupancy, seed, flags, clearance_sq = 0.1, 1, 0, 1
    sq, st, _ = _random_field(occupancy, seed, flags)
    cells = np.argwhere(T.free_of(sq, st, flags, clearance_sq))
    goals = (cells[np.random.default_rng(3).choice(len(cells), 4, replace=False)] + RANDOM_LO).astype(np.int32)
    tsdf = _table(_random_entries(occupancy, seed), log2=15)
    call = lambda g: tsdf.travel_field(RANDOM_BOX, g, clearance_sq=clearance_sq, min_weight=1, unknown_is_site=False)      # noqa: E731
    singles = [call(goals[i:i + 1]) for i in range(4)]
    assert all(s.n_goals_used == 1 and s.n_reached > 1000 for s in singles)
    together = call(goals)
    assert together.n_goals_used == 4 and np.array_equal(together.cost, np.minimum.reduce([s.cost for s in singles]))
    assert any((together.cost != s.cost).any() for s in singles)
    assert call(np.concatenate([goals, goals[::-1]])).n_goals_used == 8          # a cell named twice counts twice and changes nothing
    assert np.array_equal(call(np.concatenate([goals, goals[::-1]])).cost, together.cost)
    tsdf.close()


# ---- a fused map ---------------------------------------------------------------------------------------------------------------------
FUSED_TRAVEL_SHAPE = (36, 24, 84)


@functools.lru_cache(maxsize=None)
def _fused_travel_reference():
    """(entries, box, goals, {flags: the restatement's field}): the frames of the field test, the box from the first camera's voxel
    towards the scene, the goal that voxel."""
    e, _ = _fused_reference()
    (_, _, pose), _ = _fused_frames()
    cam = np.floor(pose[:3, 3] / 0.2).astype(np.int64)
    lo = cam - [FUSED_TRAVEL_SHAPE[0] // 2, FUSED_TRAVEL_SHAPE[1] // 2, 3]
    box = _box([int(v) for v in lo], FUSED_TRAVEL_SHAPE)
    goals = cam[None].astype(np.int32)
    want = {flags: T.travel(e, FUSED_MIN_WEIGHT, box, flags, 1, goals) for flags in (0, F.UNKNOWN_IS_SITE)}
    return e, box, goals, want


@pytest.mark.parametrize("flags", (0, F.UNKNOWN_IS_SITE))
@pytest.mark.parametrize("gray", (False, True), ids=("plain", "gray"))
def test_fused_map_against_the_restatement(viso, gray, flags):
    e, box, goals, want = _fused_travel_reference()
    tsdf = libviso_amd.TsdfMap(None, gray=gray, voxel=0.2, capacity_log2=21)
    for d, img, pose in _fused_frames():
        if gray:
            tsdf.fuse(d, _param(), pose=pose, image=img)
        else:
            tsdf.fuse(d, _param(), pose=pose)
    assert tsdf.entries().tobytes() == e.tobytes()
    _check(tsdf, want[flags], box, flags, 1, goals, min_weight=FUSED_MIN_WEIGHT)
    tsdf.close()


# ---- the call reads only, and says what the distance field says -----------------------------------------------------------------------
@pytest.mark.parametrize("gray", (False, True), ids=("plain", "gray"))
def test_consistency(viso, gray):
    e = TT.random_block(np.random.default_rng(9))
    tsdf = _table(e, log2=10, gray=gray)
    before, st = tsdf.entries(gray=gray).tobytes(), tsdf.stats()
    box, goals = ([-7, -6, -8], [8, 7, 6]), [[-7, -6, -8], [7, 6, 5], [0, 0, 0]]
    for flags in (0, F.UNKNOWN_IS_SITE):
        for mw in (1, 2):
            want = T.travel(e, mw, box, flags, 1, goals)
            a = _check(tsdf, want, box, flags, 1, goals, min_weight=mw)
            b = _check(tsdf, want, box, flags, 1, goals, min_weight=mw)            # two calls in a row
            assert a.cost.tobytes() == b.cost.tobytes() and (a.n_goals_used, a.n_reached) == (b.n_goals_used, b.n_reached)
            d = tsdf.distance_field(box, min_weight=mw, unknown_is_site=bool(flags))
            assert a.field.sq.tobytes() == d.sq.tobytes() and a.field.state.tobytes() == d.state.tobytes() and a.field.n_sites == d.n_sites
    assert tsdf.entries(gray=gray).tobytes() == before and tsdf.stats() == st
    tsdf.close()


# ---- refusals behind a live handle ---------------------------------------------------------------------------------------------------
def test_refusals_behind_a_live_handle(viso):
    L = viso
    e = TT.random_block(np.random.default_rng(9))
    tsdf = _table(e, log2=10)
    box = VoxelBox((C.c_int32 * 3)(-4, -4, -4), (C.c_int32 * 3)(0, 1, 2))     # 4 x 5 x 6 cells
    goals = np.array([[-4, -4, -4], [-1, 0, 1], [9, 9, 9]], np.int32)
    cost, sq, st = np.full(120, 77, np.uint32), np.full(120, 77, np.uint32), np.full(120, 77, np.uint8)
    counts = [C.c_size_t(99) for _ in range(3)]
    u32p = C.POINTER(C.c_uint32)

    def call(handle, cap=120, with_field=True, with_counts=True):
        return L.viso_tsdf_travel_field(handle, 1, C.byref(box), 0, 0, goals.ctypes.data_as(C.POINTER(C.c_int32)), 3, cost.ctypes.data_as(u32p),
                                        sq.ctypes.data_as(u32p) if with_field else None,
                                        st.ctypes.data_as(C.POINTER(C.c_uint8)) if with_field else None, cap,
                                        *[C.byref(c) if with_counts else None for c in counts])

    untouched = lambda: (cost == 77).all() and (sq == 77).all() and (st == 77).all() and all(c.value == 99 for c in counts)      # noqa: E731
    # n_cap one short: nothing written
    assert call(tsdf.h, cap=119) == -1 and b"viso_tsdf_travel_field" in L.viso_last_error() and untouched()
    # exactly enough; without the field and without the counts
    want = T.travel(e, 1, ([-4, -4, -4], [0, 1, 2]), 0, 0, goals)
    assert call(tsdf.h) == 1
    assert cost.tobytes() == want[0].tobytes() and sq.tobytes() == want[1].tobytes() and st.tobytes() == want[2].tobytes()
    assert [c.value for c in counts[:2]] == [want[3], want[4]] and counts[2].value >= 1
    cost[:] = 77
    assert call(tsdf.h, with_field=False, with_counts=False) == 1 and cost.tobytes() == want[0].tobytes()
    cost[:], sq[:], st[:] = 77, 77, 77
    for c in counts:
        c.value = 99
    # an overflowed map refuses
    many = np.zeros(1025, R.ENTRY)
    many["k"][:, 0] = np.arange(1025) + 500
    many["weight"], many["sum"] = 1, -7
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.add_entries(many)
    assert call(tsdf.h) == -4 and b"overflowed" in L.viso_last_error() and untouched()
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.travel_field(([-4, -4, -4], [0, 1, 2]), goals)
    tsdf.clear()
    assert tsdf.travel_field(([-4, -4, -4], [0, 1, 2]), goals, min_weight=1, unknown_is_site=False).n_reached == 120
    h = tsdf.h
    tsdf.close()
    assert call(h) == -1 and b"not a live" in L.viso_last_error()            # a destroyed map
    # a map whose context is gone
    ctx = libviso_amd.Context(0)
    orphan = libviso_amd.TsdfMap(ctx, voxel=0.2, capacity_log2=10)
    orphan.add_entries(e)
    ctx.close()
    assert call(orphan.h) == -1 and b"context has been destroyed" in L.viso_last_error()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        orphan.travel_field(([-4, -4, -4], [0, 1, 2]), goals)
    assert untouched()
    orphan.close()
