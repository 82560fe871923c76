"""No-GPU checks of the TSDF travel field (include/viso_hip.h, "TSDF travel field"): the restatement (tests/travel_ref.py) against the
closed form of the open box and a hand-made serpentine; the path rule, in the restatement and in TravelField; the symbol; every
argument error that needs no device; the rounding of a clearance in metres."""
import ctypes as C
import itertools

import numpy as np
import pytest

import libviso_amd
from libviso_amd import abi
from libviso_amd.abi import VoxelBox

import travel_ref as T

NONE = T.NONE


def closed_form(shape, goal):
    """3a + b + c over the box, (a >= b >= c) the sorted absolute offsets from the goal."""
    d = np.stack(np.meshgrid(*[np.abs(np.arange(n) - g) for n, g in zip(shape, goal)], indexing="ij"), axis=-1)
    d = np.sort(d, axis=-1)
    return (3 * d[..., 2] + d[..., 1] + d[..., 0]).astype(np.uint32)


def serpentine():
    """(free [25][25][1], the cells of the openings): rows 1, 3, .., 23 blocked but for one cell, at column 24 and column 0 in turn."""
    free = np.ones((25, 25, 1), bool)
    gaps = []
    for j, row in enumerate(range(1, 24, 2)):
        free[row, :, 0] = False
        gaps.append((row, 24 if j % 2 == 0 else 0, 0))
        free[gaps[-1]] = True
    return free, gaps


def check_path(p, cost, free, start):
    """The path checks of the issue: the 26 moves between free cells, the step costs sum to cost[start], the end is a goal."""
    assert p.ndim == 2 and p.shape[1] == 3 and tuple(p[0]) == tuple(start)
    total = 0
    for a, b in zip(p[:-1], p[1:]):
        e = b - a
        assert np.abs(e).max() == 1 and free[tuple(a)] and free[tuple(b)]
        total += 2 + int((e != 0).sum())
    assert total == int(cost[tuple(start)]) and cost[tuple(p[-1])] == 0
    assert len({tuple(c) for c in p}) == len(p)


# ---- the restatement against hand values ---------------------------------------------------------------------------------------------
def test_open_box_is_the_closed_form():
    shape, goal = (9, 8, 17), (2, 7, 5)
    cost, used = T.costs(np.ones(shape, bool), [goal])
    assert used == 1 and cost.dtype == np.uint32 and np.array_equal(cost, closed_form(shape, goal))
    d = np.stack(np.meshgrid(*[np.arange(n) - g for n, g in zip(shape, goal)], indexing="ij"), axis=-1).astype(np.float64)
    euclid = np.sqrt((d * d).sum(axis=-1))
    away = euclid > 0
    ratio = cost[away] / 3.0 / euclid[away]
    assert ratio.min() >= 4 / (3 * np.sqrt(2.0)) - 1e-12 and ratio.max() <= np.sqrt(11.0) / 3 + 1e-12
    # both extremes are in the box: along (1, 1, 0) and along (3, 1, 1)
    assert np.isclose(ratio.min(), 4 / (3 * np.sqrt(2.0))) and np.isclose(ratio.max(), np.sqrt(11.0) / 3)


def test_serpentine_reaches_every_free_cell():
    free, gaps = serpentine()
    cost, used = T.costs(free, [(0, 0, 0)])
    assert used == 1 and ((cost != NONE) == free).all() and int(cost[free].max()) == 960
    # the way from the far end goes through every opening
    p = T.path(cost, (24, 24, 0))
    cells = {tuple(c) for c in p}
    assert all(g in cells for g in gaps)
    check_path(p, cost, free, (24, 24, 0))


def test_goals_that_are_skipped_and_no_goal():
    free = np.ones((4, 3, 2), bool)
    free[1] = False         # a wall: the cells beyond it are never reached
    cost, used = T.costs(free, [(0, 0, 0), (1, 1, 1), (4, 0, 0), (0, -1, 0), (0, 0, 0)])
    assert used == 2 and (cost[1:] == NONE).all() and np.array_equal(cost[0], closed_form((1, 3, 2), (0, 0, 0))[0])
    cost, used = T.costs(free, [(1, 0, 0), (7, 7, 7)])
    assert used == 0 and (cost == NONE).all()
    # several goals: the cell-wise minimum
    a, b = T.costs(free, [(0, 2, 1)])[0], T.costs(free, [(3, 0, 0)])[0]
    assert np.array_equal(T.costs(free, [(0, 2, 1), (3, 0, 0)])[0], np.minimum(a, b))


def test_free_of_is_rule_2():
    sq = np.array([0, 0, 1, 4, 9, 9, NONE, NONE, 5], np.uint32).reshape(9, 1, 1)
    st = np.array([1 | 4, 0, 1, 0, 2, 1, 0, 2, 0], np.uint8).reshape(9, 1, 1)
    free = lambda flags, c: T.free_of(sq, st, flags, c).reshape(-1).tolist()           # noqa: E731
    #                      surface unknown front  unknown behind front  unknown behind unknown
    assert free(0, 0) == [False, True, True, True, False, True, True, False, True]
    assert free(0, 5) == [False, False, False, False, False, True, True, False, True]
    assert free(1, 0) == [False, False, True, False, False, True, False, False, False]
    assert free(0, NONE - 1) == [False, False, False, False, False, False, True, False, False]


# ---- the path rule -------------------------------------------------------------------------------------------------------------------
def _field_of(free, goals, lo=(0, 0, 0), voxel=0.5):
    """A TravelField over hand-made costs: (field, cost)."""
    cost, used = T.costs(free, goals)
    lo = np.asarray(lo)
    f = libviso_amd.TravelField(cost, None, (lo, lo + np.asarray(free.shape)), voxel, 0, used, int((cost != NONE).sum()), 1)
    return f, cost


def test_path_rule():
    rng = np.random.default_rng(5)
    free = rng.random((9, 10, 11)) > 0.3
    free[0, 0, 0] = free[8, 9, 10] = True
    goals = [(0, 0, 0), (8, 9, 10)]
    lo = np.array([-4, 100, 7])
    f, cost = _field_of(free, goals, lo)
    reached = np.argwhere(cost != NONE)
    assert len(reached) > 200
    for start in reached[rng.choice(len(reached), 40, replace=False)]:
        p = T.path(cost, start)
        check_path(p, cost, free, start)
        assert tuple(p[-1]) in goals
        # the first neighbour in the order of the product: no earlier one leads on
        for a, b in zip(p[:-1], p[1:]):
            for e in T.MOVES:
                m = a + e
                if tuple(e) == tuple(b - a):
                    break
                ok = ((m >= 0) & (m < free.shape)).all() and cost[tuple(m)] != NONE
                assert not (ok and int(cost[tuple(m)]) + T.move_cost(e) == int(cost[tuple(a)]))
        got = f.path(start + lo)
        assert got.dtype == np.int32 and np.array_equal(got, p + lo)
        assert np.array_equal(f.path_metres(start + lo), (p + lo + 0.5) * 0.5)
    # None: a start that is not reached, one that is not free, one outside the box
    walled = np.ones((5, 5, 1), bool)
    walled[2] = False
    f, cost = _field_of(walled, [(0, 0, 0)])
    for start in ((4, 4, 0), (2, 3, 0), (5, 0, 0), (0, -1, 0), (0, 0, 1)):
        assert T.path(cost, start) is None and f.path(np.array(start)) is None and f.path_metres(np.array(start)) is None
    assert np.array_equal(f.path(np.array([0, 0, 0])), [[0, 0, 0]])
    with pytest.raises(ValueError):
        f.path(np.array([0.5, 0, 0]))


def test_travel_field_helpers():
    cost = np.array([[[0, 3, 7, NONE]], [[4, 5, 8, 11]]], np.uint32)
    f = libviso_amd.TravelField(cost, None, ([-1, 3, 10], [1, 4, 14]), 0.25, 2, 1, 7, 3)
    assert f.cost is cost and f.voxel == 0.25 and (f.clearance_sq, f.n_goals_used, f.n_reached, f.rounds) == (2, 1, 7, 3)
    assert f.box[0].dtype == np.int32 and f.box[0].tolist() == [-1, 3, 10] and f.box[1].tolist() == [1, 4, 14]
    m = f.metres()
    want = np.array([[[0, 0.25, 7 / 3 * 0.25, np.inf]], [[4 / 3 * 0.25, 5 / 3 * 0.25, 8 / 3 * 0.25, 11 / 3 * 0.25]]])
    assert m.dtype == np.float32 and np.array_equal(m, want.astype(np.float32))
    got, outside = f.at([[-0.25, 0.75, 2.5], [-0.01, 0.99, 3.49], [0.0, 0.8, 3.0], [0.25, 0.8, 3.0], [np.nan, 0.8, 3.0]])
    assert got.dtype == np.uint32 and got.tolist() == [0, NONE, 8, NONE, NONE] and outside.tolist() == [False, False, False, True, True]
    assert [tuple(e) for e in libviso_amd.maps.TRAVEL_MOVES] == T.MOVES == [e for e in itertools.product((-1, 0, 1), repeat=3) if any(e)]
    assert libviso_amd.maps.TRAVEL_MOVE_COSTS.tolist() == [T.move_cost(e) for e in T.MOVES]


# ---- the rounding of a clearance -----------------------------------------------------------------------------------------------------
def test_clearance_rounding():
    sq = libviso_amd.travel_clearance_sq
    assert sq(0.0, 0.2) == 0
    for voxel in (0.125, 0.25, 0.5, 1.0):     # k * voxel is exact
        for k in (1, 2, 3, 7, 100, 511):
            c = k * voxel
            assert sq(c, voxel) == k * k, (voxel, k)                                # an exact square
            assert sq(np.nextafter(c, np.inf), voxel) == k * k + 1, (voxel, k)      # a hair above: the next integer
            assert sq(np.nextafter(c, 0.0), voxel) == k * k, (voxel, k)             # a hair below k voxels: up to k^2
    assert sq(0.75, 0.25) == 9 and sq(0.76, 0.25) == 10
    assert sq(0.25 * 1.5, 0.25) == 3          # 2.25 voxels^2: up to 3
    assert sq(0.25 * np.sqrt(2.0), 0.25) == 3  # the double nearest to sqrt 2 squares to a hair above 2
    assert sq(1e-9, 0.2) == 1                 # any clearance above 0 asks for sq >= 1
    # the rule is about the two doubles as they are: 0.6 lies below three times the double 0.2, 0.9 above three times the double 0.3
    assert sq(0.6, 0.2) == 9 and sq(0.9, 0.3) == 10
    for bad in ((-0.1, 0.2), (np.nan, 0.2), (np.inf, 0.2), (1.0, 0.0), (1.0, -1.0), (1e9, 1e-3)):
        with pytest.raises(ValueError):
            sq(*bad)


def test_python_argument_checks_need_no_library():
    class Stub:
        h, L, voxel = None, None, 0.2
    call = libviso_amd.TsdfMap.travel_field.fget(Stub())
    box = ([0, 0, 0], [4, 4, 4])
    with pytest.raises(ValueError, match="1 .. 512"):
        call(([0, 0, 0], [1, 513, 1]), [[0, 0, 0]])
    with pytest.raises(ValueError, match="either goals"):
        call(box)
    with pytest.raises(ValueError, match="either goals"):
        call(box, [[0, 0, 0]], goals_m=[[0.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match=r"\[n\]\[3\]"):
        call(box, [[0, 0]])
    with pytest.raises(ValueError, match=r"\[n\]\[3\]"):
        call(box, [[0.0, 0.0, 0.0]])
    with pytest.raises(ValueError, match="finite"):
        call(box, goals_m=[[0.0, np.nan, 0.0]])
    with pytest.raises(ValueError, match="int32"):
        call(box, [[0, 0, 1 << 31]])
    with pytest.raises(ValueError, match="either clearance or clearance_sq"):
        call(box, [[0, 0, 0]], clearance=0.5, clearance_sq=4)
    with pytest.raises(ValueError, match="uint32"):
        call(box, [[0, 0, 0]], clearance_sq=-1)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    return libviso_amd.load()


def test_symbol_is_declared_and_exported(L):
    fn = L.viso_tsdf_travel_field
    assert fn.restype is C.c_int
    u32p, szp = C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)
    assert fn.argtypes == [C.c_void_p, C.c_uint32, C.POINTER(VoxelBox), C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.c_size_t, u32p, u32p,
                           C.POINTER(C.c_uint8), C.c_size_t, szp, szp, szp]
    assert abi.PROTOTYPES["tsdf_travel_field"] == (fn.restype, fn.argtypes)


def _box(lo, hi):
    return VoxelBox((C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi))


def test_argument_errors_need_no_device(L):
    """Every check of the arguments comes before the handle is looked at, and the handle before a device: with a handle that is
    not a map, each of them is reached.  A refused call writes nothing."""
    cost, sq, st = np.full(8, 77, np.uint32), np.full(8, 77, np.uint32), np.full(8, 77, np.uint8)
    counts = [C.c_size_t(99) for _ in range(3)]
    good = _box([0, 0, 0], [2, 2, 2])
    one = np.zeros((1, 3), np.int32)
    many = np.zeros((65537, 3), np.int32)

    def call(handle=None, min_weight=1, box=good, flags=0, clearance_sq=0, goals=one, n_goals=1, out=cost, cap=8):
        r = L.viso_tsdf_travel_field(handle, min_weight, C.byref(box) if box is not None else None, flags, clearance_sq,
                                     goals.ctypes.data_as(C.POINTER(C.c_int32)) if goals is not None else None, n_goals,
                                     out.ctypes.data_as(C.POINTER(C.c_uint32)) if out is not None else None,
                                     sq.ctypes.data_as(C.POINTER(C.c_uint32)), st.ctypes.data_as(C.POINTER(C.c_uint8)), cap,
                                     *[C.byref(c) for c in counts])
        return r, L.viso_last_error()

    cases = {
        "min_weight 0": dict(min_weight=0), "null box": dict(box=None), "null cost_out": dict(out=None),
        "flag 2": dict(flags=2), "flag 3": dict(flags=3), "flag 2^31": dict(flags=1 << 31),
        "clearance_sq NONE": dict(clearance_sq=NONE), "null goals": dict(goals=None),
        "n_goals 0": dict(n_goals=0), "n_goals 65537": dict(goals=many, n_goals=65537),
        "empty axis": dict(box=_box([0, 0, 0], [2, 0, 2])), "513 voxels": dict(box=_box([0, 0, -13], [1, 1, 500]), cap=1 << 20),
        "n_cap one short": dict(cap=7), "n_cap 0": dict(cap=0),
        "null handle": dict(), "not a map": dict(handle=C.addressof(counts[0])),
        "not a map, every goal": dict(handle=C.addressof(counts[0]), goals=many[:65536], n_goals=65536, flags=1, clearance_sq=NONE - 1),
    }
    for name, kw in cases.items():
        r, err = call(**kw)
        assert r == abi.VISO_ERR_ARG, (name, r, err)
        assert b"viso_tsdf_travel_field" in err, (name, err)
        assert (b"not a live TSDF handle" in err) == ("handle" in name or "not a map" in name), (name, err)
    assert (cost == 77).all() and (sq == 77).all() and (st == 77).all() and all(c.value == 99 for c in counts)      # nothing written


def test_interface_reports_the_error():
    m = libviso_amd.TsdfMap.__new__(libviso_amd.TsdfMap)       # a map that was never created
    m.L, m.h, m.voxel = libviso_amd.load(), None, 0.2
    with pytest.raises(libviso_amd.VisoError, match="viso_tsdf_travel_field: not a live TSDF handle"):
        m.travel_field(([0, 0, 0], [2, 2, 2]), [[0, 0, 0]])
    with pytest.raises(libviso_amd.VisoError, match="min_weight >= 1"):
        m.travel_field(([0, 0, 0], [2, 2, 2]), [[0, 0, 0]], min_weight=0)
    with pytest.raises(libviso_amd.VisoError, match="clearance_sq below VISO_FIELD_NONE"):
        m.travel_field(([0, 0, 0], [2, 2, 2]), [[0, 0, 0]], clearance_sq=NONE)


# ---- the tool's flags ----------------------------------------------------------------------------------------------------------------
def test_tool_flags_need_their_modes(capsys):
    from libviso_amd import fuse_map
    base = ["d", "p", "c", "o.ply"]
    for argv in (base + ["--travel-field", "t.npz"], base + ["--surface", "--travel-clearance", "0.5"],
                 base + ["--surface", "--travel-field", "t.npz", "--travel-clearance", "-1"],
                 base + ["--mesh", "--travel-field", "t.npz", "--travel-clearance", "nan"],
                 base + ["--mesh", "--travel-field", "t.npz", "--field-half-side", "-1"]):
        with pytest.raises(SystemExit) as e:
            fuse_map.main(argv)
        assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--travel-field needs --surface or --mesh" in err and "--travel-clearance needs --travel-field" in err
    assert "--travel-clearance needs a clearance >= 0" in err and "--field-half-side needs a half side >= 0" in err
