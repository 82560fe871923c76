"""The opt-in semi-global matching on the device (include/viso_hip.h, viso_stereo_sgm / viso_batch_set_sgm;
libviso_amd/csrc/sgm.hip) against its numpy restatement (tests/sgm_ref.py), in the batch over workspace groups, beside the
image-in pipeline and behind on-device rectification."""
import itertools

import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MatchParams

import sgm_ref as SR
from test_gpu_disparity import _pair
from test_sgm_cpu import largest_cost_pair

pytestmark = pytest.mark.gpu


def _prm(D, paths, pp, u, m):
    return dict(num_disp=D, paths=paths, p1=pp[0], p2=pp[1], uniqueness=u, lr_max_diff=m)


# the whole product of the parameter edges, on small images
SWEEP = [_prm(*c) for c in itertools.product((16, 64, 128, 256), (4, 8), ((1, 1), (10, 120), (192, 192)), (0, 10, 100), (-1, 0, 1))]


@pytest.mark.parametrize("D", (16, 64, 128, 256))
def test_device_equals_restatement_over_parameters(viso, D):
    rng = np.random.default_rng(100 + D)
    L, R = _pair(rng, 24, 150 if D < 256 else 300)
    for p in (q for q in SWEEP if q["num_disp"] == D):
        assert np.array_equal(libviso_amd.stereo_sgm(L, R, **p), SR.sgm(L, R, **p)), p


@pytest.mark.parametrize("D", (48, 80, 144, 176, 208))
def test_disparity_counts_between_the_lane_multiples(viso, D):
    """D that do not fill the lanes' K disparities (K = ceil(D / 64))."""
    rng = np.random.default_rng(D)
    L, R = _pair(rng, 17, 260)
    for paths in (4, 8):
        assert np.array_equal(libviso_amd.stereo_sgm(L, R, num_disp=D, paths=paths), SR.sgm(L, R, num_disp=D, paths=paths))


@pytest.mark.parametrize("shape,params", [
    ((376, 1241), dict()),
    ((376, 1241), dict(paths=4, num_disp=64, uniqueness=0, lr_max_diff=-1)),
    ((37, 333), dict(num_disp=32)),
    ((1, 1), dict()),
    ((1, 50), dict(num_disp=16)),
    ((50, 1), dict(num_disp=16)),
    ((3, 5), dict(num_disp=16)),                 # smaller than the census window
    ((25, 100), dict(num_disp=256)),             # D > cols
    ((21, 2048), dict(num_disp=64)),             # the widest this build handles
])
def test_device_equals_restatement_over_geometries(viso, shape, params):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    L, R = _pair(rng, *shape) if shape[1] > 8 else (rng.integers(0, 256, shape).astype(np.uint8), rng.integers(0, 256, shape).astype(np.uint8))
    for m in ((1, -1) if shape[0] < 100 else (None,)):
        p = dict(params) if m is None else dict(params, lr_max_diff=m)
        assert np.array_equal(libviso_amd.stereo_sgm(L, R, **p), SR.sgm(L, R, **p)), p


def test_largest_costs_and_a_constant_pair(viso):
    yy, xx = np.mgrid[0:30, 0:90]
    checker = (((xx + yy) & 1) * 255).astype(np.uint8)
    stripes = ((xx & 1) * 255).astype(np.uint8)
    const = np.full((30, 90), 77, np.uint8)
    dots, zero = largest_cost_pair(30, 90)   # C = 62
    for L, R in ((dots, zero), (zero, dots), (checker, 255 - checker), (stripes, 255 - stripes), (checker, stripes), (const, const), (const, checker)):
        for p in (dict(num_disp=16, p1=192, p2=192), dict(num_disp=32, uniqueness=0, lr_max_diff=-1), dict(num_disp=16, paths=4, p1=1, p2=1)):
            assert np.array_equal(libviso_amd.stereo_sgm(L, R, **p), SR.sgm(L, R, **p)), p
    for u in (0, 10, 100):   # d* = 0 everywhere, and unique (tests/test_sgm_cpu.py::test_constant_image)
        assert (libviso_amd.stereo_sgm(const, const, num_disp=16, uniqueness=u) == 0).all()


def test_slanted_plane_accuracy_on_the_device(viso):
    """The restatement's own figures (tests/test_sgm_cpu.py): 0.985 valid, median 0.095 px, 0.24 % beyond 1 px."""
    L, R, dtrue = SR.slanted_pair()
    d = libviso_amd.stereo_sgm(L, R)
    valid, med, big = SR.accuracy(d, dtrue)
    print(f"device: valid {valid:.3f} median {med:.3f} px > 1 px {big:.4f}")
    assert np.array_equal(d, SR.sgm(L, R))
    assert abs(valid - 0.985) <= 0.02 and med <= 1.5 * 0.095 and abs(big - 0.0024) <= 0.02 and big <= 0.01 and valid >= 0.95


def test_valid_shares_on_the_subpixel_sequence(viso):
    """The shares of valid pixels on the flat noisy background of make_subpixel_image_sequence: defaults 0.573, m = -1 0.726,
    u = 0 and m = -1 1.0, the device equal to the restatement."""
    seq = synth.make_subpixel_image_sequence(2, 2, n_kp=1500)
    L, R = seq["images"][1]
    shares = []
    for p in (dict(), dict(lr_max_diff=-1), dict(uniqueness=0, lr_max_diff=-1)):
        d = libviso_amd.stereo_sgm(L, R, **p)
        assert np.array_equal(d, SR.sgm(L, R, **p))
        shares.append(float((d != SR.INVALID).mean()))
    print("valid shares (defaults, m = -1, u = 0 and m = -1):", shares)
    assert all(abs(s - w) <= 0.02 for s, w in zip(shares, (0.573, 0.726, 1.0))), shares


def _seq():
    return synth.make_subpixel_image_sequence(4, 6, n_kp=500, width=640, height=200)


def _run(ctx, seq, sgm, seed=3, matcher_only=False):
    nf, cap = seq["kp"].shape[0], seq["kp"].shape[2]
    b = libviso_amd.Batch(ctx, nf, cap)
    b.upload_images(seq["images"], seq["kp"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=seed)
    b.set_covariance(1)
    b.set_refine(1)
    b.set_window_refine(3)
    if sgm is not None:
        b.set_sgm(sgm)
    b.run_images(matcher_only=matcher_only)
    return b


def test_batch_equals_direct_and_leaves_the_pipeline_untouched(viso):
    seq = _seq()
    ctx = libviso_amd.Context(0)
    ref = _run(ctx, seq, None)
    prm = dict(num_disp=64, p1=7, p2=86)
    b = _run(ctx, seq, prm)
    nf = seq["kp"].shape[0]
    all_d = b.disparities()
    for t in range(nf):
        want = libviso_amd.stereo_sgm(seq["images"][t, 0], seq["images"][t, 1], **prm)
        assert np.array_equal(b.disparity(t), want) and np.array_equal(all_d[t], want)
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
    # matcher_only runs compute it too, and leave the matches as they are without it
    b.set_sgm(num_disp=16, paths=4)
    b.run_images(matcher_only=True)
    assert np.array_equal(b.disparity(2), libviso_amd.stereo_sgm(seq["images"][2, 0], seq["images"][2, 1], num_disp=16, paths=4))
    mo = _run(ctx, seq, None, matcher_only=True)
    for t in range(nf):
        for which in range(3 if t else 1):
            assert np.array_equal(b.matches(which, t), mo.matches(which, t))
    with pytest.raises(TypeError):
        b.set_sgm(libviso_amd.sgm_params(), paths=4)
    # off: the getters refuse
    b.set_sgm(None)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.disparity(0)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.run_disparity()
    b.close(); ref.close(); mo.close(); ctx.close()


def test_workspace_groups_give_the_same_maps(viso):
    """Five frames through groups of 5, 2 and 1 (a cap of exactly one frame); a cap below one frame is VISO_ERR_NOMEM."""
    rng = np.random.default_rng(11)
    shape, D = (40, 200), 32
    imgs = np.stack([np.stack(_pair(rng, *shape)) for _ in range(5)])
    want = np.stack([libviso_amd.stereo_sgm(imgs[t, 0], imgs[t, 1], num_disp=D) for t in range(5)])
    assert np.array_equal(want[3], SR.sgm(imgs[3, 0], imgs[3, 1], num_disp=D))
    per = libviso_amd.sgm_frame_bytes(*shape, D)
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 5, 64)
    b.set_sgm(num_disp=D)
    b.upload_images_only(imgs)
    try:
        for cap in (0, 2 * per + per // 2, per):
            libviso_amd.sgm_set_workspace_cap(cap)
            b.run_disparity()
            assert np.array_equal(b.disparities(), want), cap
        libviso_amd.sgm_set_workspace_cap(per - 1)
        with pytest.raises(libviso_amd.VisoError, match="-4"):
            b.run_disparity()
        with pytest.raises(libviso_amd.VisoError, match="-4"):
            libviso_amd.stereo_sgm(imgs[0, 0], imgs[0, 1], num_disp=D)
        libviso_amd.sgm_set_workspace_cap(per)
        b.run_disparity()   # the batch stays usable
        assert np.array_equal(b.disparity(4), want[4])
    finally:
        libviso_amd.sgm_set_workspace_cap(0)
    b.close(); ctx.close()


def test_run_disparity_without_keypoints_and_geometry_growth(viso):
    rng = np.random.default_rng(7)
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 3, 64)
    b.set_sgm(num_disp=32, paths=4)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.run_disparity()   # no images
    for shape in ((40, 120), (60, 333)):   # the images grow after set_sgm: the maps and the workspace follow
        imgs = np.stack([np.stack(_pair(rng, *shape)) for _ in range(3)])
        b.upload_images_only(imgs)
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b.disparity(0)   # nothing computed yet for this geometry
        b.run_disparity()
        d = b.disparities()
        assert d.shape == (3,) + shape
        for t in range(3):
            assert np.array_equal(d[t], SR.sgm(imgs[t, 0], imgs[t, 1], num_disp=32, paths=4))
    with pytest.raises(libviso_amd.VisoError):
        b.set_sgm(num_disp=20)
    b.close(); ctx.close()


def test_one_method_at_a_time(viso):
    rng = np.random.default_rng(5)
    imgs = np.stack([np.stack(_pair(rng, 40, 160)) for _ in range(2)])
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 2, 64)
    b.upload_images_only(imgs)
    b.set_disparity(num_disp=32, block=7)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.set_sgm(num_disp=32)
    b.run_disparity()   # still the block matcher's
    bm = libviso_amd.stereo_disparity(imgs[1, 0], imgs[1, 1], num_disp=32, block=7)
    assert np.array_equal(b.disparity(1), bm)
    b.set_disparity(None)
    b.set_sgm(num_disp=32)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.set_disparity(num_disp=32, block=7)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.disparity(1)   # the block matcher's maps are not SGM's
    b.run_disparity()
    assert np.array_equal(b.disparity(1), libviso_amd.stereo_sgm(imgs[1, 0], imgs[1, 1], num_disp=32))
    # another batch's block matching is untouched by this one's SGM
    b2 = libviso_amd.Batch(ctx, 2, 64)
    b2.upload_images_only(imgs)
    b2.set_disparity(num_disp=32, block=7)
    b2.run_disparity()
    assert np.array_equal(b2.disparity(1), bm)
    b.close(); b2.close(); ctx.close()


def test_descriptor_in_run_refuses_and_the_batch_stays_usable(viso, oracle):
    seq = synth.make_sequence(4, 4, n_kp=400, width=500, height=200)
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 4, 400)
    b.upload(seq["kp"], seq["desc"], seq["n"])
    b.set_params(st, tm, seq["param"], seed=1)
    b.set_sgm({})
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.run()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.run_matcher()
    b.set_sgm(None)
    b.run()
    tr, ok, n_inl = b.poses()
    want = oracle.sequence(seq["kp"], seq["desc"], seq["n"], st, tm, seq["param"], seed=1)
    assert np.array_equal(ok, want["ok"]) and np.array_equal(n_inl, want["n_inl"])
    b.close(); ctx.close()


def test_rectified_images_are_what_the_kernels_read(viso):
    calib = synth.raw_stereo_calib(3, raw_shape=(250, 730), out_shape=(200, 640))
    rng = np.random.default_rng(9)
    raw = rng.integers(0, 256, (2, 2) + tuple(calib["raw_shape"])).astype(np.uint8)
    out_shape = tuple(calib["out_shape"])
    maps = [libviso_amd.rectify_map(calib["K"][s], calib["D"][s], calib["R"][s], calib["P"][s], out_shape) for s in range(2)]
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 2, 64)
    b.set_rectify(calib["raw_shape"], out_shape, left=maps[0], right=maps[1])
    b.set_sgm(num_disp=48)
    b.upload_images_only(raw)
    b.run_disparity()
    for t in range(2):
        want = libviso_amd.stereo_sgm(b.image(t, 0), b.image(t, 1), num_disp=48)
        assert np.array_equal(b.disparity(t), want)
    b.close(); ctx.close()


def test_too_wide_and_bad_parameters(viso):
    img = np.zeros((4, 2049), np.uint8)
    with pytest.raises(libviso_amd.VisoError, match="-3"):
        libviso_amd.stereo_sgm(img, img, num_disp=16)
    img = np.zeros((8, 40), np.uint8)
    for bad in (dict(num_disp=8), dict(num_disp=272), dict(num_disp=24), dict(p1=0), dict(p1=121), dict(p2=193), dict(paths=6),
                dict(uniqueness=101), dict(lr_max_diff=-2), dict(num_disp=16, lr_max_diff=17)):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.stereo_sgm(img, img, **bad)
