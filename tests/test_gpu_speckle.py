"""The opt-in speckle filter on the device (include/viso_hip.h, viso_filter_speckles / viso_batch_set_speckle;
libviso_amd/csrc/speckle.hip) against its numpy restatement (tests/speckle_ref.py): parameters, geometries around the kernel's
64 x 16 tile, shapes that stress the merge, the two methods' real maps, the batch over workspace groups, beside the image-in
pipeline and behind on-device rectification."""
import itertools

import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MatchParams

import disparity_ref as DR
import speckle_ref as K
from test_gpu_disparity import _pair
from test_speckle_cpu import DIFFS, random_map

pytestmark = pytest.mark.gpu

INV = K.INVALID
TW, TH = 64, 16   # SPK_TW, SPK_TH of speckle.hip


def _check(m, size, diff, what=None):
    got = libviso_amd.filter_speckles(m, max_size=size, max_diff=diff)
    assert np.array_equal(got, K.speckles(m, size, diff)), (what, m.shape, size, diff)


@pytest.mark.parametrize("seed", range(4))
def test_device_equals_restatement_over_parameters(viso, seed):
    rng = np.random.default_rng(seed)
    rows, cols = int(rng.integers(20, 60)), int(rng.integers(70, 200))
    m = random_map(rng, rows, cols)
    for diff, size in itertools.product(DIFFS, (0, 1, 2, 100, rows * cols)):
        _check(m, size, diff)


GEOMETRIES = [(376, 1241), (37, 333), (1, 1), (1, 50), (50, 1), (21, 2048)] + [
    (r, c) for r in (TH - 1, TH, TH + 1) for c in (TW - 1, TW, TW + 1)] + [(2 * TH + 1, 3 * TW - 1), (2 * TH, 2 * TW)]


@pytest.mark.parametrize("shape", GEOMETRIES)
def test_device_equals_restatement_over_geometries(viso, shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    for spread, invalid in ((3, 0.3), (40, 0.1), (2, 0.45)):
        m = random_map(rng, *shape, spread=spread, invalid=invalid)
        for size, diff in ((100, 16), (5, 1), (shape[0] * shape[1], 0)):
            _check(m, size, diff)


def _shapes():
    R, C = 376, 1241
    yield "serpentine", K.serpentine(R, C)
    yield "vertical serpentine", K.serpentine(R, C, vertical=True)
    yield "spiral", K.spiral(R, C)
    yield "comb", K.comb(R, C)
    yield "tile corners", K.corner_crosser(R, C, TW, TH)
    yield "constant", (np.full((R, C), 320, np.int16), R * C)


@pytest.mark.parametrize("k", range(6))
def test_shapes_that_stress_the_merge(viso, k):
    """One component each, of a known size n: kept whole for S = n - 1, removed whole for S = n."""
    name, (m, n) = list(_shapes())[k]
    assert m.shape == (376, 1241) and (m != INV).sum() == n
    got = libviso_amd.filter_speckles(m, max_size=n - 1, max_diff=0)
    assert np.array_equal(got, m), name
    got = libviso_amd.filter_speckles(m, max_size=n, max_diff=0)
    assert (got == INV).all(), name
    # with noise beside it: single pixels in the gaps that must not join it (values more than max_diff away)
    rng = np.random.default_rng(k)
    noisy = m.copy()
    gaps = (m == INV) & (rng.random(m.shape) < 0.2)
    noisy[gaps] = 2000
    for size in (100, n - 1):
        _check(noisy, size, 16, name)


def test_many_one_pixel_components(viso):
    """More than 10^5 components of one pixel (a checkerboard of valid and invalid pixels), and the same of two values."""
    yy, xx = np.mgrid[0:376, 0:1241]
    m = np.where((yy + xx) & 1, 100, INV).astype(np.int16)
    assert (m != INV).sum() > 100000
    assert (libviso_amd.filter_speckles(m, max_size=1, max_diff=4096) == INV).all()
    assert np.array_equal(libviso_amd.filter_speckles(m, max_size=0, max_diff=4096), m)
    m2 = np.where((yy + xx) & 1, 100, 117).astype(np.int16)
    assert (libviso_amd.filter_speckles(m2, max_size=1, max_diff=16) == INV).all()
    assert np.array_equal(libviso_amd.filter_speckles(m2, max_size=376 * 1241 - 1, max_diff=17), m2)


def test_real_maps_of_both_methods(viso):
    L, R, _ = DR.slanted_pair()
    seq = synth.make_subpixel_image_sequence(2, 2, n_kp=1500)
    for a, b in ((L, R), tuple(seq["images"][1])):
        for d in (libviso_amd.stereo_disparity(a, b), libviso_amd.stereo_sgm(a, b)):
            got = libviso_amd.filter_speckles(d)
            assert np.array_equal(got, K.speckles(d, 100, 16))
            print(f"valid {float((d != INV).mean()):.4f} -> {float((got != INV).mean()):.4f}")


def _seq():
    return synth.make_subpixel_image_sequence(4, 6, n_kp=500, width=640, height=200)


def _run(ctx, seq, method, speckle, seed=3, matcher_only=False):
    nf, cap = seq["kp"].shape[0], seq["kp"].shape[2]
    b = libviso_amd.Batch(ctx, nf, cap)
    b.upload_images(seq["images"], seq["kp"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=seed)
    b.set_covariance(1)
    b.set_refine(1)
    b.set_window_refine(3)
    if method == "bm":
        b.set_disparity(num_disp=64)
    elif method == "sgm":
        b.set_sgm(num_disp=64, p1=7, p2=86)
    if speckle is not None:
        b.set_speckle(speckle)
    b.run_images(matcher_only=matcher_only)
    return b


def _same_pipeline(b, ref, nf):
    for got, want in zip(b.poses(), ref.poses()):
        assert np.array_equal(got, want)
    for t in range(nf):
        for which in range(3 if t else 1):
            assert np.array_equal(b.matches(which, t), ref.matches(which, t))
        c1, c2 = b.circle(t), ref.circle(t)
        assert np.array_equal(c1[0], c2[0]) and np.array_equal(c1[1], c2[1])
    assert b.covariances().tobytes() == ref.covariances().tobytes()
    assert b.refines().tobytes() == ref.refines().tobytes()
    assert b.window_refines().tobytes() == ref.window_refines().tobytes()


@pytest.mark.parametrize("method", ("bm", "sgm"))
def test_batch_equals_direct_and_leaves_the_pipeline_untouched(viso, method):
    seq = _seq()
    nf = seq["kp"].shape[0]
    ctx = libviso_amd.Context(0)
    never = _run(ctx, seq, None, None)          # a batch that never heard of dense maps
    plain = _run(ctx, seq, method, None)        # the method alone
    prm = dict(max_size=60, max_diff=12)
    b = _run(ctx, seq, method, prm)
    raw, all_d = plain.disparities(), b.disparities()
    removed = 0
    for t in range(nf):
        want = libviso_amd.filter_speckles(raw[t], **prm)
        assert np.array_equal(want, K.speckles(raw[t], 60, 12))
        assert np.array_equal(b.disparity(t), want) and np.array_equal(all_d[t], want)
        removed += int((want != raw[t]).sum())
    assert removed > 0   # the filter had something to do
    _same_pipeline(b, never, nf)
    _same_pipeline(plain, never, nf)
    # off again: the maps are the method's own, byte for byte
    b.set_speckle(None)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.disparity(0)   # the filtered maps are not the unfiltered state's
    b.run_images()
    assert np.array_equal(b.disparities(), raw)
    # max_size 0 is valid and changes nothing
    b.set_speckle(max_size=0)
    b.run_images(matcher_only=True)
    assert np.array_equal(b.disparities(), raw)
    # matcher_only runs filter too
    b.set_speckle(prm)
    b.run_images(matcher_only=True)
    assert np.array_equal(b.disparity(2), libviso_amd.filter_speckles(raw[2], **prm))
    with pytest.raises(TypeError):
        b.set_speckle(libviso_amd.speckle_params(), max_size=4)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.set_speckle(max_diff=4097)
    b.close(); plain.close(); never.close(); ctx.close()


def test_set_speckle_with_no_method_does_nothing(viso):
    seq = _seq()
    nf = seq["kp"].shape[0]
    ctx = libviso_amd.Context(0)
    never = _run(ctx, seq, None, None)
    b = _run(ctx, seq, None, dict(max_size=60))
    _same_pipeline(b, never, nf)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.disparity(0)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.run_disparity()
    # a method turned on later is filtered
    b.set_disparity(num_disp=32, block=7)
    b.run_images()
    want = libviso_amd.filter_speckles(libviso_amd.stereo_disparity(seq["images"][1, 0], seq["images"][1, 1], num_disp=32, block=7), max_size=60)
    assert np.array_equal(b.disparity(1), want)
    b.close(); never.close(); ctx.close()


@pytest.mark.parametrize("method", ("bm", "sgm"))
def test_workspace_groups_give_the_same_maps(viso, method):
    """Five frames through groups of 5, 2 and 1 (a cap of exactly one frame); a cap below one frame is VISO_ERR_NOMEM."""
    rng = np.random.default_rng(11)
    shape = (40, 200)
    imgs = np.stack([np.stack(_pair(rng, *shape)) for _ in range(5)])
    direct = (lambda a, c: libviso_amd.stereo_disparity(a, c, num_disp=32, block=7)) if method == "bm" else (
        lambda a, c: libviso_amd.stereo_sgm(a, c, num_disp=32))
    prm = dict(max_size=30, max_diff=8)
    want = np.stack([K.speckles(direct(imgs[t, 0], imgs[t, 1]), 30, 8) for t in range(5)])
    per = libviso_amd.speckle_frame_bytes(*shape)
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 5, 64)
    if method == "bm":
        b.set_disparity(num_disp=32, block=7)
    else:
        b.set_sgm(num_disp=32)
    b.set_speckle(prm)
    b.upload_images_only(imgs)
    try:
        for cap in (0, 2 * per + per // 2, per):
            libviso_amd.speckle_set_workspace_cap(cap)
            b.run_disparity()
            assert np.array_equal(b.disparities(), want), cap
        libviso_amd.speckle_set_workspace_cap(per - 1)
        with pytest.raises(libviso_amd.VisoError, match="-4"):
            b.run_disparity()
        with pytest.raises(libviso_amd.VisoError, match="-4"):
            libviso_amd.filter_speckles(want[0], **prm)
        libviso_amd.speckle_set_workspace_cap(per)
        b.run_disparity()   # the batch stays usable
        assert np.array_equal(b.disparity(4), want[4])
    finally:
        libviso_amd.speckle_set_workspace_cap(0)
    b.close(); ctx.close()


def test_geometry_growth_after_set_speckle(viso):
    rng = np.random.default_rng(7)
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 3, 64)
    b.set_speckle(max_size=40)
    b.set_sgm(num_disp=32, paths=4)
    for shape in ((40, 120), (70, 333), (30, 90)):   # the images change after set_speckle: the maps and the workspace follow
        imgs = np.stack([np.stack(_pair(rng, *shape)) for _ in range(3)])
        b.upload_images_only(imgs)
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b.disparity(0)   # nothing computed yet for this geometry
        b.run_disparity()
        d = b.disparities()
        assert d.shape == (3,) + shape
        for t in range(3):
            assert np.array_equal(d[t], K.speckles(libviso_amd.stereo_sgm(imgs[t, 0], imgs[t, 1], num_disp=32, paths=4), 40, 16))
    b.close(); ctx.close()


def test_behind_on_device_rectification(viso):
    calib = synth.raw_stereo_calib(3, raw_shape=(250, 730), out_shape=(200, 640))
    rng = np.random.default_rng(9)
    raw = rng.integers(0, 256, (2, 2) + tuple(calib["raw_shape"])).astype(np.uint8)
    out_shape = tuple(calib["out_shape"])
    maps = [libviso_amd.rectify_map(calib["K"][s], calib["D"][s], calib["R"][s], calib["P"][s], out_shape) for s in range(2)]
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 2, 64)
    b.set_rectify(calib["raw_shape"], out_shape, left=maps[0], right=maps[1])
    b.set_disparity(num_disp=48)
    b.set_speckle({})
    b.upload_images_only(raw)
    b.run_disparity()
    for t in range(2):
        want = K.speckles(libviso_amd.stereo_disparity(b.image(t, 0), b.image(t, 1), num_disp=48), 100, 16)
        assert np.array_equal(b.disparity(t), want)
    b.close(); ctx.close()


def test_too_wide_and_bad_parameters(viso):
    with pytest.raises(libviso_amd.VisoError, match="-3"):
        libviso_amd.filter_speckles(np.zeros((4, 2049), np.int16))
    m = np.zeros((8, 40), np.int16)
    for bad in (dict(max_size=-1), dict(max_diff=-1), dict(max_diff=4097)):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.filter_speckles(m, **bad)
    keep = m.copy()
    libviso_amd.filter_speckles(m, max_size=8 * 40)
    assert np.array_equal(m, keep)   # the caller's array is not written
