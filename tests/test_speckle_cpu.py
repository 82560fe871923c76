"""The speckle filter and the reprojection of include/viso_hip.h without a device: the two numpy restatements
(tests/speckle_ref.py) against each other, known answers, the argument checks of the C ABI, the struct layout, the effect of the
filter on the two methods' maps, and the kernels' resource usage."""
import ctypes as C
import itertools

import numpy as np
import pytest

import libviso_amd
from libviso_amd import hostmath, synth
from libviso_amd.abi import SPECKLE_DEFAULTS, Param, SpeckleParams

import disparity_ref as DR
import sgm_ref as SR
import speckle_ref as K
from estimator_util import kernel_resources

INV = K.INVALID
DIFFS = (0, 1, 16, 4096)


def random_map(rng, rows, cols, spread=None, invalid=None):
    """Random values in [0, spread) with a random share invalid."""
    spread = int(rng.choice((2, 6, 40, 2000, 8000))) if spread is None else spread
    invalid = rng.random() * 0.7 if invalid is None else invalid
    m = rng.integers(0, spread, (rows, cols)).astype(np.int16)
    m[rng.random((rows, cols)) < invalid] = INV
    return m


@pytest.mark.parametrize("seed", range(6))
def test_vectorised_equals_flood_fill(seed):
    rng = np.random.default_rng(seed)
    rows, cols = int(rng.integers(1, 24)), int(rng.integers(1, 40))
    m = random_map(rng, rows, cols)
    for diff, size in itertools.product(DIFFS, (0, 1, 2, 100, rows * cols)):
        assert np.array_equal(K.speckles(m, size, diff), K.speckles_loop(m, size, diff)), (diff, size)


def test_known_answers():
    rows, cols = 7, 9
    n = rows * cols
    # all invalid
    m = np.full((rows, cols), INV, np.int16)
    assert np.array_equal(K.speckles(m, 5, 16), m)
    # constant: one component of rows * cols pixels
    m = np.full((rows, cols), 200, np.int16)
    assert np.array_equal(K.speckles(m, n - 1, 0), m)
    assert (K.speckles(m, n, 0) == INV).all()
    # checkerboard of two values more than max_diff apart: every pixel its own component
    yy, xx = np.mgrid[0:rows, 0:cols]
    m = np.where((yy + xx) & 1, 100, 117).astype(np.int16)
    assert (K.speckles(m, 1, 16) == INV).all() and (K.speckles(m, n, 16) == INV).all()
    assert np.array_equal(K.speckles(m, 0, 16), m)
    assert np.array_equal(K.speckles(m, 0, 17), m) and np.array_equal(K.speckles(m, n - 1, 17), m)   # 17 apart, max_diff 17: one component
    # a component of exactly S and one of exactly S + 1 pixels side by side
    S = 6
    m = np.full((4, 9), INV, np.int16)
    m[0:2, 0:3] = 50            # 6 pixels
    m[0, 4:9] = 50; m[1, 4:6] = 50   # 7 pixels; column 3 separates them
    out = K.speckles(m, S, 0)
    assert (out[0:2, 0:3] == INV).all() and np.array_equal(out[:, 4:], m[:, 4:])
    assert np.array_equal(K.speckles(m, S - 1, 0), m) and (K.speckles(m, S + 1, 0) == INV).all()
    # side by side with different values, touching
    m = np.full((2, 7), 50, np.int16)
    m[:, 3:] = 500              # 6 and 8 pixels, neighbours but not linked
    out = K.speckles(m, 6, 16)
    assert (out[:, :3] == INV).all() and (out[:, 3:] == 500).all()
    # a chain p - q - r: links are between neighbours, not to a seed
    m = np.array([[100, 110, 120]], np.int16)
    assert np.array_equal(K.component_sizes(m, 10), [[3, 3, 3]])
    assert np.array_equal(K.speckles(m, 2, 10), m) and (K.speckles(m, 3, 10) == INV).all()
    assert np.array_equal(K.component_sizes(m, 9), [[1, 1, 1]])
    # two regions that touch only diagonally
    m = np.full((4, 4), INV, np.int16)
    m[0:2, 0:2] = 80
    m[2:4, 2:4] = 80
    assert np.array_equal(K.component_sizes(m, 16)[m != INV], np.full(8, 4))
    assert (K.speckles(m, 4, 16) == INV).all() and np.array_equal(K.speckles(m, 3, 16), m)
    # negative values other than the invalid one are ordinary values
    m = np.array([[-15, -17, -16, -1]], np.int16)
    assert np.array_equal(K.component_sizes(m, 2), [[2, 2, 0, 1]])


def test_stress_shapes_are_one_component():
    for m, n in (K.serpentine(21, 40), K.serpentine(40, 21, vertical=True), K.spiral(23, 31), K.comb(12, 33), K.corner_crosser(50, 200, 64, 16)):
        assert K.component_sizes(m, 0).max() == n == (m != INV).sum()
        assert np.array_equal(K.speckles(m, n - 1, 0), m) and (K.speckles(m, n, 0) == INV).all()
        assert np.array_equal(K.speckles(m, n, 0), K.speckles_loop(m, n, 0))


def test_params_struct_and_defaults():
    assert [f[0] for f in SpeckleParams._fields_] == ["max_size", "max_diff"] and C.sizeof(SpeckleParams) == 8
    L = libviso_amd.load()
    p = SpeckleParams(-1, -1)
    L.viso_speckle_params_default(C.byref(p))
    assert (p.max_size, p.max_diff) == (100, 16) == (SPECKLE_DEFAULTS["max_size"], SPECKLE_DEFAULTS["max_diff"])
    L.viso_speckle_params_default(None)
    q = libviso_amd.speckle_params(max_size=7)
    assert (q.max_size, q.max_diff) == (7, 16) and q.ok()
    with pytest.raises(TypeError):
        libviso_amd.speckle_params(foo=1)
    with pytest.raises(TypeError):
        libviso_amd.disparity_params(max_size=1)   # not a field of the methods' structs
    assert libviso_amd.speckle_frame_bytes(376, 1241) == 2 * ((376 * 1241 * 4 + 255) // 256 * 256)


def test_argument_errors_without_a_device():
    L = libviso_amd.load()
    m = np.zeros((4, 5), np.int16)
    mp = m.ctypes.data_as(C.POINTER(C.c_int16))
    ok = SpeckleParams(100, 16)
    assert L.viso_filter_speckles(None, 4, 5, C.byref(ok)) == -1
    assert L.viso_filter_speckles(mp, 4, 5, None) == -1
    for rows, cols in ((0, 5), (4, 0), (-1, 5)):
        assert L.viso_filter_speckles(mp, rows, cols, C.byref(ok)) == -1
    for bad in ((-1, 16), (100, -1), (100, 4097)):
        p = SpeckleParams(*bad)
        assert not p.ok() and L.viso_filter_speckles(mp, 4, 5, C.byref(p)) == -1
        assert b"viso_filter_speckles" in L.viso_last_error()
    wide = np.zeros((1, 2049), np.int16)
    assert L.viso_filter_speckles(wide.ctypes.data_as(C.POINTER(C.c_int16)), 1, 2049, C.byref(ok)) == -3
    # max_size 0 changes nothing: no device is needed
    assert L.viso_filter_speckles(mp, 4, 5, C.byref(SpeckleParams(0, 16))) == 1 and not m.any()
    # a cap below one frame
    L.viso_speckle_set_workspace_cap(libviso_amd.speckle_frame_bytes(4, 5) - 1)
    try:
        assert L.viso_filter_speckles(mp, 4, 5, C.byref(ok)) == -4
    finally:
        L.viso_speckle_set_workspace_cap(0)
    assert L.viso_batch_set_speckle(None, C.byref(ok)) == -1 and L.viso_batch_set_speckle(None, None) == -1
    assert L.viso_batch_get_disparity_points(None, 0, None, 1, None) == -1
    # the reprojection
    prm = Param.default(base=0.5, f=700.0, cu=600.5, cv=180.25)
    out = np.zeros((4, 5, 3), np.float32)
    op = out.ctypes.data_as(C.POINTER(C.c_float))
    assert L.viso_disparity_to_points(None, 4, 5, C.byref(prm), None, 1, op) == -1
    assert L.viso_disparity_to_points(mp, 4, 5, None, None, 1, op) == -1
    assert L.viso_disparity_to_points(mp, 4, 5, C.byref(prm), None, 1, None) == -1
    assert L.viso_disparity_to_points(mp, 0, 5, C.byref(prm), None, 1, op) == -1
    assert L.viso_disparity_to_points(mp, 4, 0, C.byref(prm), None, 1, op) == -1
    assert L.viso_disparity_to_points(mp, 4, 5, C.byref(prm), None, 0, op) == -1
    assert b"viso_disparity_to_points" in L.viso_last_error()
    with pytest.raises(ValueError):
        libviso_amd.filter_speckles(np.zeros((4, 5), np.int32))
    with pytest.raises(ValueError):
        libviso_amd.disparity_to_points(m, prm, pose=np.eye(3))


def test_points_restatement():
    prm = Param.default(base=0.5, f=700.0, cu=2.5, cv=1.25)
    m = np.full((3, 6), INV, np.int16)
    m[2, 5] = 40      # d = 2.5 px
    m[0, 0] = 0       # a disparity of 0: below every min_disp16
    m[1, 1] = 15
    m[1, 2] = 16
    P = K.points(m, prm)
    want = np.array([0.5 * (5 - 2.5) / 2.5, 0.5 * (2 - 1.25) / 2.5, 700.0 * 0.5 / 2.5], np.float32)
    assert np.array_equal(P[2, 5], want) and np.array_equal(want, np.array([0.5, 0.15, 140.0], np.float32))
    assert np.isnan(P[0, 0]).all() and np.isnan(P[0, 1]).all() and np.isfinite(P[1, 1]).all()
    P16 = K.points(m, prm, min_disp16=16)
    assert np.isnan(P16[1, 1]).all() and np.isfinite(P16[1, 2]).all() and np.array_equal(P16[2, 5], want)
    assert K.points_equal(K.points(m, prm, pose=np.eye(4)), P)          # identity equals no pose (x * 1 + 0 terms are exact)
    T = np.linalg.inv(hostmath.tr2mat([0.01, -0.02, 0.005, 0.3, -0.1, 1.5]))
    Q = K.points(m, prm, pose=T)
    X = P[2, 5].astype(np.float64)
    assert np.allclose(Q[2, 5], T[:3, :3] @ X + T[:3, 3], rtol=1e-6) and not K.points_equal(Q, P)
    assert K.points_equal(Q, K.points(m, prm, pose=T[:3]))


def _effect(name, d, dtrue, p):
    out = K.speckles(d, p["max_size"], p["max_diff"])
    v0, v1 = d != INV, out != INV
    line = f"{name}: valid {v0.mean():.4f} -> {v1.mean():.4f}"
    if dtrue is not None:
        e0 = (np.abs(d[v0] / 16.0 - dtrue[v0]) > 1.0).mean()
        e1 = (np.abs(out[v1] / 16.0 - dtrue[v1]) > 1.0).mean() if v1.any() else 0.0
        line += f", valid pixels more than 1 px off {e0:.5f} -> {e1:.5f}"
    print(line)
    # what follows from the definition
    assert not (v1 & ~v0).any() and np.array_equal(out[v1], d[v1])
    sz = K.component_sizes(out, p["max_diff"])
    assert (sz[v1] > p["max_size"]).all()
    return out


def test_effect_on_both_methods_maps():
    """The shares before and after the filter with defaults (DESIGN.md 5.13 carries the printed figures; they are measured, not
    pinned).  Asserted: the filtered valid set is a subset of the unfiltered one, kept pixels keep their values, and no component of
    at most max_size pixels remains (removing whole components never makes a new small one: the kept components are untouched)."""
    p = SPECKLE_DEFAULTS
    L, R, dtrue = DR.slanted_pair()
    _effect("slanted pair, block matching", DR.disparity(L, R), dtrue, p)
    _effect("slanted pair, SGM", SR.sgm(L, R), dtrue, p)
    seq = synth.make_subpixel_image_sequence(2, 2, n_kp=1500)
    L, R = seq["images"][1]
    _effect("synthetic frame 1, block matching", DR.disparity(L, R), None, p)
    _effect("synthetic frame 1, SGM", SR.sgm(L, R), None, p)


def test_kernels_have_no_scratch():
    names = ("speckle_tile_kernel", "speckle_border_kernel", "speckle_count_kernel", "speckle_apply_kernel", "points_kernel")
    res = kernel_resources("speckle.hip", names)
    for name, (occ, scratch) in res.items():
        print(f"{name}: occupancy {occ}, scratch {scratch}")
        assert scratch == 0 and occ >= 1


def test_device_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    m = np.zeros((30, 40), np.int16)
    with pytest.raises(libviso_amd.VisoError, match="-2"):
        libviso_amd.filter_speckles(m)
    with pytest.raises(libviso_amd.VisoError, match="-2"):
        libviso_amd.disparity_to_points(m, Param.default(base=0.5, f=700.0, cu=20.0, cv=15.0))
