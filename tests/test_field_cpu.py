"""No-GPU checks of the TSDF distance field (include/viso_hip.h, "TSDF distance field"): the restatement (tests/field_ref.py) against
hand values and, where scipy is installed, against its exact Euclidean transform; the DistanceField helpers; the symbol; every
argument error, none of which needs a device; the tool's flags."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd import abi, fuse_map
from libviso_amd.abi import VoxelBox

import field_ref as F
import tsdf_ref as R

BIAS = 1 << 20


def _entries(rows):
    """[(k, weight, sum)] as a TSDF entry array sorted by key."""
    e = np.zeros(len(rows), R.ENTRY)
    for i, (k, w, s) in enumerate(rows):
        e["k"][i], e["weight"][i], e["sum"][i] = k, w, s
    return e[np.argsort(R.keys_of(e["k"]))]


# ---- the restatement against hand values ---------------------------------------------------------------------------------------------
def test_one_site_in_a_corner():
    # the voxel at the box's corner in front, its partner behind it outside the box
    e = _entries([((0, 0, 0), 2, 10), ((-1, 0, 0), 2, -10)])
    box = ([0, 0, 0], [4, 3, 5])
    sq, st, n = F.field(e, 1, box)
    i, j, k = np.meshgrid(np.arange(4), np.arange(3), np.arange(5), indexing="ij")
    assert n == 1 and sq.dtype == np.uint32 and np.array_equal(sq, i * i + j * j + k * k)
    want = np.zeros((4, 3, 5), np.uint8)
    want[0, 0, 0] = 1 | F.SURFACE
    assert st.dtype == np.uint8 and np.array_equal(st, want)
    # the same box moved so that both ends are inside: two sites, next to each other along axis 0
    sq, st, n = F.field(e, 1, ([-1, 0, 0], [3, 3, 5]))
    assert n == 2 and np.array_equal(sq, np.minimum(i * i, (i - 1) * (i - 1)) + j * j + k * k)
    assert st[0, 0, 0] == 2 | F.SURFACE and st[1, 0, 0] == 1 | F.SURFACE
    # with the unknown cells as sites, every cell but none is a site
    sq, st, n = F.field(e, 1, box, F.UNKNOWN_IS_SITE)
    assert n == 60 and not sq.any()


def test_two_equidistant_sites_and_no_site():
    # crossings along axis 1 whose ends in the box are the cells 0 and 6 of a line of 7
    e = _entries([((5, -1, 5), 1, -3), ((5, 0, 5), 1, 0), ((5, 6, 5), 3, -1), ((5, 7, 5), 1, 7)])
    sq, st, n = F.field(e, 1, ([5, 0, 5], [6, 7, 6]))
    assert n == 2 and sq.reshape(-1).tolist() == [0, 1, 4, 9, 4, 1, 0]
    assert st.reshape(-1).tolist() == [1 | F.SURFACE, 0, 0, 0, 0, 0, 2 | F.SURFACE]         # sum == 0 is in front
    # min_weight 2: three of the four are unknown, no crossing is left
    sq, st, n = F.field(e, 2, ([5, 0, 5], [6, 7, 6]))
    assert n == 0 and (sq == F.NONE).all() and st.reshape(-1).tolist() == [0, 0, 0, 0, 0, 0, 2]
    sq, st, n = F.field(e, 2, ([5, 0, 5], [6, 7, 6]), F.UNKNOWN_IS_SITE)
    assert n == 6 and sq.reshape(-1).tolist() == [0, 0, 0, 0, 0, 0, 1]
    # an empty table
    sq, st, n = F.field(e[:0], 1, ([-3, 0, 9], [0, 2, 11]))
    assert n == 0 and sq.shape == (3, 2, 2) and (sq == F.NONE).all() and not st.any()


def test_key_range_ends_have_no_neighbour_and_nothing_wraps():
    # an entry at the last index and one of the other sign at the first: no neighbours of each other
    e = _entries([((BIAS - 1, 0, 0), 1, 5), ((-BIAS, 0, 0), 1, -5)])
    sq, st, n = F.field(e, 1, ([BIAS - 2, 0, 0], [BIAS + 2, 1, 1]))
    assert n == 0 and st.reshape(-1).tolist() == [0, 1, 0, 0]
    sq, st, n = F.field(e, 1, ([BIAS - 2, 0, 0], [BIAS + 2, 1, 1]), F.UNKNOWN_IS_SITE)
    assert n == 3 and sq.reshape(-1).tolist() == [0, 1, 0, 0]
    sq, st, n = F.field(e, 1, ([-(1 << 31), 0, 0], [-(1 << 31) + 3, 1, 1]))
    assert n == 0 and not st.any()


def test_brute_force_forms_agree():
    rng = np.random.default_rng(1)
    for shape, p in (((7, 5, 9), 0.05), ((3, 11, 4), 0.3), ((1, 1, 13), 0.2), ((6, 1, 1), 0.0)):
        site = rng.random(shape) < p
        assert np.array_equal(F.brute(site), F.brute_loop(site)), shape
        assert np.array_equal(F.brute(site, chunk=7), F.brute(site))


def test_restatement_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2)
    for shape, p in (((33, 29, 67), 0.01), ((12, 40, 9), 0.2), ((512, 1, 1), 0.004)):
        site = rng.random(shape) < p
        assert site.any()
        edt = ndimage.distance_transform_edt(~site)
        assert np.array_equal(np.rint(edt * edt).astype(np.uint32), F.brute(site)), shape


# ---- the Python helpers ------------------------------------------------------------------------------------------------------------
def test_distance_field_helpers():
    sq = np.array([[[0, 1, 4, 9]], [[1, 2, 5, abi.FIELD_NONE]]], np.uint32)
    st = np.array([[[1 | 4, 1, 2, 0]], [[2, 2, 0, 0]]], np.uint8)
    f = libviso_amd.DistanceField(sq, st, ([-1, 3, 10], [1, 4, 14]), 0.25, 1)
    assert f.sq is sq and f.state is st and f.voxel == 0.25 and f.n_sites == 1
    assert f.box[0].dtype == np.int32 and f.box[0].tolist() == [-1, 3, 10] and f.box[1].tolist() == [1, 4, 14]
    m = f.metres()
    want = np.array([[[0, 0.25, 0.5, 0.75]], [[0.25, np.sqrt(2.0) * 0.25, np.sqrt(5.0) * 0.25, np.inf]]])
    assert m.dtype == np.float32 and np.array_equal(m, want.astype(np.float32))
    s = f.signed_metres()
    assert s.dtype == np.float32 and np.array_equal(s, (want * [[[1, 1, -1, 1]], [[-1, -1, 1, 1]]]).astype(np.float32))
    # points: the cell is floor(p / voxel) - lo
    pts = [[-0.25, 0.75, 2.5], [-0.01, 0.99, 3.49], [0.0, 0.8, 3.0], [0.2, 0.76, 3.26], [0.25, 0.8, 3.0], [0.0, 1.0, 3.0], [0.0, 0.8, 2.49],
           [np.nan, 0.8, 3.0], [-0.26, 0.8, 3.0]]
    got, outside = f.at(pts)
    assert got.dtype == np.uint32 and outside.dtype == bool
    assert outside.tolist() == [False, False, False, False, True, True, True, True, True]
    assert got.tolist() == [0, 9, 5, abi.FIELD_NONE] + [abi.FIELD_NONE] * 5
    with pytest.raises(ValueError):
        f.at([1.0, 2.0, 3.0])
    assert abi.FIELD_UNKNOWN_IS_SITE == F.UNKNOWN_IS_SITE and abi.FIELD_NONE == F.NONE and abi.FIELD_STATE_SURFACE == F.SURFACE


def test_python_box_checks_need_no_library():
    class Stub:          # the call checks the box before it reaches the handle
        h, L, voxel = None, None, 0.2
    call = libviso_amd.TsdfMap.distance_field.fget(Stub())
    for box in (([0, 0, 0], [0, 1, 1]), ([0, 0, 0], [1, 513, 1]), ([5, 0, 0], [4, 1, 1])):
        with pytest.raises(ValueError, match="1 .. 512"):
            call(box)
    with pytest.raises(ValueError, match="int32"):
        call(([0, 0, 0], [1, 1, 1 << 31]))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    return libviso_amd.load()


def test_symbol_is_declared_and_exported(L):
    fn = L.viso_tsdf_distance_field
    assert fn.restype is C.c_int
    assert fn.argtypes == [C.c_void_p, C.c_uint32, C.POINTER(VoxelBox), C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8),
                           C.c_size_t, C.POINTER(C.c_size_t)]
    assert abi.PROTOTYPES["tsdf_distance_field"] == (fn.restype, fn.argtypes)


def _box(lo, hi):
    return VoxelBox((C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi))


def test_argument_errors_need_no_device(L):
    """Every check of the arguments comes before the handle is looked at, and the handle before a device: with a handle that is
    not a map, each of them is reached."""
    sq = np.full(8, 77, np.uint32)
    st = np.full(8, 77, np.uint8)
    n = C.c_size_t(99)
    good = _box([0, 0, 0], [2, 2, 2])
    i32 = (-(1 << 31), (1 << 31) - 1)

    def call(handle=None, min_weight=1, box=good, flags=0, out=sq, cap=8):
        r = L.viso_tsdf_distance_field(handle, min_weight, C.byref(box) if box is not None else None, flags,
                                       out.ctypes.data_as(C.POINTER(C.c_uint32)) if out is not None else None,
                                       st.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(n))
        return r, L.viso_last_error()

    cases = {
        "min_weight 0": dict(min_weight=0), "null box": dict(box=None), "null sq_out": dict(out=None),
        "flag 2": dict(flags=2), "flag 3": dict(flags=3), "flag 2^31": dict(flags=1 << 31),
        "empty axis": dict(box=_box([0, 0, 0], [2, 0, 2])), "negative axis": dict(box=_box([0, 5, 0], [2, 4, 2])),
        "513 voxels": dict(box=_box([0, 0, -13], [1, 1, 500]), cap=1 << 20),
        "2^32 - 1 voxels": dict(box=_box([i32[0]] * 3, [i32[1]] * 3), cap=1 << 20),
        "n_cap one short": dict(cap=7), "n_cap 0": dict(cap=0),
        "n_cap one short of 512^2": dict(box=_box([0, 0, 0], [512, 512, 1]), cap=512 * 512 - 1),
        "null handle": dict(), "not a map": dict(handle=C.addressof(n)),
        "not a map, flagged": dict(handle=C.addressof(n), flags=1),
    }
    for name, kw in cases.items():
        r, err = call(**kw)
        assert r == abi.VISO_ERR_ARG, (name, r, err)
        assert b"viso_tsdf_distance_field" in err, (name, err)
        assert (b"not a live TSDF handle" in err) == ("handle" in name or "not a map" in name), (name, err)
    assert (sq == 77).all() and (st == 77).all() and n.value == 99      # nothing written


def test_interface_reports_the_error():
    m = libviso_amd.TsdfMap.__new__(libviso_amd.TsdfMap)       # a map that was never created
    m.L, m.h, m.voxel = libviso_amd.load(), None, 0.2
    with pytest.raises(libviso_amd.VisoError, match="viso_tsdf_distance_field: not a live TSDF handle"):
        m.distance_field(([0, 0, 0], [2, 2, 2]))
    with pytest.raises(libviso_amd.VisoError, match="min_weight >= 1"):
        m.distance_field(([0, 0, 0], [2, 2, 2]), min_weight=0)


# ---- the tool's flags --------------------------------------------------------------------------------------------------------------
def test_tool_flags_need_their_modes(capsys):
    base = ["d", "p", "c", "o.ply"]
    for argv in (base + ["--distance-field", "f.npz"], base + ["--surface", "--field-half-side", "5"],
                 base + ["--mesh", "--distance-field", "f.npz", "--field-half-side", "-1"],
                 base + ["--mesh", "--distance-field", "f.npz", "--field-half-side", "nan"]):
        with pytest.raises(SystemExit) as e:
            fuse_map.main(argv)
        assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--distance-field needs --surface or --mesh" in err and "--field-half-side needs --distance-field" in err
    assert "--field-half-side needs a half side >= 0" in err


def test_tool_box_is_clipped_to_the_longest_field():
    (lo, hi), clipped = fuse_map.field_box([1.0, 2.0, 300.0], 20.0, 0.2)
    want = libviso_amd.voxel_box([1.0, 2.0, 300.0], 20.0, 0.2)
    assert not clipped and np.array_equal(lo, want[0]) and np.array_equal(hi, want[1]) and (hi - lo <= 512).all()
    (lo, hi), clipped = fuse_map.field_box([1.0, 2.0, 300.0], 200.0, 0.2)
    assert clipped and (hi - lo == 512).all() and lo.tolist() == [5 - 256, 10 - 256, 1500 - 256]
    (lo, hi), clipped = fuse_map.field_box([1.0, -0.1, 300.0], 51.3, 0.2)       # 514 voxels: one axis' worth over
    assert clipped and (hi - lo == 512).all()
    (lo, hi), clipped = fuse_map.field_box([0.0, 0.0, 0.0], 51.0, 0.2)          # 511 voxels
    assert not clipped and (hi - lo == 511).all()
