"""The semi-global matching of include/viso_hip.h without a device: the numpy restatement (tests/sgm_ref.py) against its literal
per-pixel form, hand cases, the bound on S, the parameter ranges, the accuracy of the defaults, and the kernels' resource usage."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import SGM_DEFAULTS, SgmParams

import sgm_ref as SR
from estimator_util import kernel_resources


def _pair(rng, rows, cols, shift=5):
    base = rng.integers(0, 256, (rows, cols + shift)).astype(np.int32)
    base = (base + np.roll(base, 1, 1) + np.roll(base, 1, 0)) // 3
    R = base[:, :cols].copy()
    R[:, cols // 3:cols // 3 + 5] = rng.integers(0, 256, (rows, 5))
    return base[:, shift:shift + cols].astype(np.uint8), R.astype(np.uint8)


def largest_cost_pair(rows=16, cols=40):
    yy, xx = np.mgrid[0:rows, 0:cols]
    return (((xx % 5 == 0) & (yy % 4 == 0)) * 255).astype(np.uint8), np.zeros((rows, cols), np.uint8)


EDGES = [dict(paths=paths, uniqueness=u, lr_max_diff=m) for paths in (4, 8) for u in (0, 10, 100) for m in (-1, 0, 1)] + [
    dict(p1=7, p2=7), dict(p1=1, p2=1, paths=4), dict(p1=10, p2=192), dict(p1=192, p2=192), dict(lr_max_diff=16), dict(num_disp=32)]


@pytest.mark.parametrize("k", range(len(EDGES)))
def test_vectorised_equals_loop(k):
    rng = np.random.default_rng(k)
    L, R = _pair(rng, 20, 48)
    p = dict(dict(num_disp=16), **EDGES[k])
    a, sa = SR.sgm(L, R, with_smax=True, **p)
    b, sb = SR.sgm_loop(L, R, with_smax=True, **p)
    assert np.array_equal(a, b) and sa == sb, p


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (3, 5), (7, 9)])
def test_vectorised_equals_loop_on_tiny_images(shape):
    rng = np.random.default_rng(shape[0] * 10 + shape[1])
    L, R = rng.integers(0, 256, shape).astype(np.uint8), rng.integers(0, 256, shape).astype(np.uint8)
    for p in (dict(num_disp=16), dict(num_disp=16, paths=4, uniqueness=0, lr_max_diff=-1)):
        assert np.array_equal(SR.sgm(L, R, **p), SR.sgm_loop(L, R, **p))


def test_census_bits():
    img = np.array([[5, 1], [9, 5]], np.uint8)
    c = SR.census(img)
    # (0, 0): the window's clamped pixels are 5 (x <= 0, y <= 0), 1 (x > 0, y <= 0), 9 (x <= 0, y > 0), 5; only the 1s are smaller
    assert bin(int(c[0, 0])).count("1") == 4 * 4          # columns +1..+4, rows -3..0
    assert bin(int(c[0, 1])).count("1") == 0              # 1 is the smallest value
    assert bin(int(c[1, 0])).count("1") == 62 - (5 * 4 - 1)   # every pixel but the 9s (columns -4..0, rows 0..+3, itself excluded)
    assert int(c.max()) < 1 << 62


def test_constant_image():
    """Every C = 0 and d* = 0 everywhere.  The sums are not all 0: d = x is a candidate of p but not of p - (1, 0), so the rightward
    path (and the two diagonals that come from the left) reach it only through d - 1 and pay P1, and L_r(., d) keeps that P1 for
    every d >= 1 from there on.  So S(0) = 0 < P1 <= S(d >= 1): d* = 0 is unique and every pixel is valid for every u."""
    img = np.full((12, 30), 200, np.uint8)
    C = SR.cost_volume(img, img, 16)
    assert (C[C < SR.BIG] == 0).all()
    for paths in (4, 8):
        S, smax = SR.sum_volume(img, img, 16, 10, 120, paths)
        assert (S[:, :, 0] == 0).all() and (S[:, 1:, 1] >= 10).all() and smax <= paths * 120   # M + P2 caps every L_r
        for u in (0, 10, 100):
            for m in (-1, 0):
                assert (SR.sgm(img, img, num_disp=16, paths=paths, uniqueness=u, lr_max_diff=m) == 0).all()


def test_integer_shift_is_recovered():
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, (24, 100)).astype(np.uint8)
    shift = 6
    L, R = base[:, :-shift].copy(), base[:, shift:].copy()   # L(x) = R(x - shift)
    d = SR.sgm(L, R, num_disp=16)
    inner = d[:, shift + 4:-4].astype(np.int32)
    assert (inner != SR.INVALID).mean() > 0.99
    assert (np.abs(inner[inner != SR.INVALID] - 16 * shift) <= 8).all()   # d* = shift; the V-fit moves it by half a pixel at most
    assert (SR.sgm(L, R, num_disp=16, uniqueness=0, lr_max_diff=-1)[:, shift + 4:-4] + 8 >> 4 == shift).all()


def test_sum_bound():
    """S <= paths (62 + P2), reached or not.  A lattice of single 255 pixels on 0 (every one the strict maximum of its window:
    all 62 bits) against a constant image (no bit) reaches C = 62."""
    L, Z = largest_cost_pair()
    C = SR.cost_volume(L, Z, 16)
    assert int(C[C < SR.BIG].max()) == 62
    yy, xx = np.mgrid[0:16, 0:40]
    checker = (((xx + yy) & 1) * 255).astype(np.uint8)
    rng = np.random.default_rng(2)
    for P1, P2 in ((1, 1), (10, 120), (192, 192)):
        for paths in (4, 8):
            for A, B in ((L, Z), (checker, 255 - checker), _pair(rng, 16, 40)):
                _, smax = SR.sum_volume(A, B, 16, P1, P2, paths)
                print(f"P1 {P1} P2 {P2} paths {paths}: largest S {smax}, bound {paths * (62 + P2)}")
                assert smax <= paths * (62 + P2)


def test_parameter_ranges():
    assert SR.check_params(**SR.DEFAULTS) and SR.DEFAULTS == SGM_DEFAULTS
    good = [dict(), dict(num_disp=16), dict(num_disp=256), dict(p1=1), dict(p1=120), dict(p2=192), dict(p1=192, p2=192), dict(paths=4),
            dict(uniqueness=0), dict(uniqueness=100), dict(lr_max_diff=-1), dict(lr_max_diff=128), dict(num_disp=16, lr_max_diff=16)]
    bad = [dict(num_disp=0), dict(num_disp=8), dict(num_disp=24), dict(num_disp=272), dict(p1=0), dict(p1=121), dict(p2=9), dict(p2=193),
           dict(paths=0), dict(paths=5), dict(paths=16), dict(uniqueness=-1), dict(uniqueness=101), dict(lr_max_diff=-2),
           dict(lr_max_diff=129), dict(num_disp=16, lr_max_diff=17)]
    for p in good:
        assert libviso_amd.sgm_params(**p).ok() and SR.check_params(**dict(SR.DEFAULTS, **p)), p
    for p in bad:
        assert not libviso_amd.sgm_params(**p).ok() and not SR.check_params(**dict(SR.DEFAULTS, **p)), p
    with pytest.raises(TypeError):
        libviso_amd.sgm_params(block=11)
    lib = libviso_amd.load()
    d = SgmParams()
    lib.viso_sgm_params_default(C.byref(d))
    assert {k: getattr(d, k) for k in SGM_DEFAULTS} == SGM_DEFAULTS


def test_arguments_are_checked_before_any_device():
    """VISO_ERR_ARG / _UNSUPPORTED come back on a machine without a GPU too: the checks precede the first device call."""
    img = np.zeros((8, 40), np.uint8)
    for bad in (dict(num_disp=24), dict(p1=0), dict(p2=193), dict(paths=6), dict(uniqueness=101), dict(lr_max_diff=-2)):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.stereo_sgm(img, img, **bad)
    wide = np.zeros((2, 2049), np.uint8)
    with pytest.raises(libviso_amd.VisoError, match="-3"):
        libviso_amd.stereo_sgm(wide, wide)
    lib = libviso_amd.load()
    p = libviso_amd.sgm_params()
    assert lib.viso_stereo_sgm(None, None, 8, 40, C.byref(p), None) == -1
    assert lib.viso_batch_set_sgm(None, C.byref(p)) == -1
    try:
        libviso_amd.sgm_set_workspace_cap(libviso_amd.sgm_frame_bytes(8, 40, 128) - 1)
        with pytest.raises(libviso_amd.VisoError, match="-4"):
            libviso_amd.stereo_sgm(img, img)
    finally:
        libviso_amd.sgm_set_workspace_cap(0)


def test_slanted_plane_accuracy_of_the_defaults():
    """Measured with this restatement: 0.985 valid, median 0.095 px, 0.24 % of the valid pixels beyond 1 px.  A
    valid share below 0.95 or more than 1 % beyond 1 px would mean the restatement is wrong."""
    L, R, dtrue = SR.slanted_pair()
    d, smax = SR.sgm(L, R, with_smax=True)
    valid, med, big = SR.accuracy(d, dtrue)
    print(f"restatement: valid {valid:.4f} median {med:.4f} px > 1 px {big:.5f} largest S {smax}")
    assert smax <= 8 * (62 + 120)
    assert valid >= 0.95 and big <= 0.01
    assert abs(valid - 0.985) <= 0.02 and abs(big - 0.0024) <= 0.02 and med <= 1.5 * 0.095


def test_kernels_have_no_scratch():
    names = ("sgm_census_kernel", "sgm_select_kernel") + tuple(f"sgm_path_kernelILi{k}E" for k in (1, 2, 3, 4))
    res = kernel_resources("sgm.hip", names)
    for name, (occ, scratch) in res.items():
        print(f"{name}: occupancy {occ}, scratch {scratch}")
        assert scratch == 0 and occ >= 1


def test_device_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    img = np.zeros((30, 40), np.uint8)
    with pytest.raises(libviso_amd.VisoError, match="-2"):
        libviso_amd.stereo_sgm(img, img)
