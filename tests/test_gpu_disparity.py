"""The opt-in dense stereo disparity on the device (include/viso_hip.h, viso_stereo_disparity / viso_batch_set_disparity;
libviso_amd/csrc/disparity.hip) against its numpy restatement (tests/disparity_ref.py), in the batch, beside the image-in
pipeline and behind on-device rectification."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MatchParams

import disparity_ref as DR
from test_disparity_cpu import largest_cost_pair

pytestmark = pytest.mark.gpu


def _pair(rng, rows, cols, shift=9):
    """A textured pair with a horizontal shift, some noise and a band of unrelated texture (every rule has work)."""
    base = rng.integers(0, 256, (rows, cols + shift)).astype(np.int32)
    base = (base + np.roll(base, 1, 1) + np.roll(base, 1, 0)) // 3
    L = base[:, shift:shift + cols].copy()
    R = base[:, :cols].copy()
    R[:, cols // 3:cols // 3 + 7] = rng.integers(0, 256, (rows, min(7, cols)))[:, :R[:, cols // 3:cols // 3 + 7].shape[1]]
    R = np.clip(R + rng.normal(scale=2.0, size=R.shape), 0, 255)
    return L.astype(np.uint8), R.astype(np.uint8)


PARAMS = [
    dict(num_disp=16, block=5, prefilter_cap=1, texture_threshold=0, uniqueness=0, lr_max_diff=-1),
    dict(num_disp=64, block=11, prefilter_cap=31, texture_threshold=10, uniqueness=15, lr_max_diff=1),
    dict(num_disp=128, block=21, prefilter_cap=63, texture_threshold=5000, uniqueness=100, lr_max_diff=0),
    dict(num_disp=256, block=5, prefilter_cap=63, texture_threshold=10, uniqueness=15, lr_max_diff=0),
    dict(num_disp=16, block=21, prefilter_cap=31, texture_threshold=0, uniqueness=100, lr_max_diff=1),
    dict(num_disp=64, block=5, prefilter_cap=1, texture_threshold=20, uniqueness=15, lr_max_diff=-1),
    dict(num_disp=256, block=11, prefilter_cap=31, texture_threshold=0, uniqueness=0, lr_max_diff=1),
    dict(num_disp=128, block=11, prefilter_cap=1, texture_threshold=10, uniqueness=100, lr_max_diff=-1),
]


@pytest.mark.parametrize("k", range(len(PARAMS)))
def test_device_equals_restatement_over_parameters(viso, k):
    rng = np.random.default_rng(100 + k)
    L, R = _pair(rng, 48, 301)
    got = libviso_amd.stereo_disparity(L, R, **PARAMS[k])
    assert np.array_equal(got, DR.disparity(L, R, **PARAMS[k]))


@pytest.mark.parametrize("shape,params", [
    ((376, 1241), dict()),
    ((37, 333), dict(num_disp=32, block=7)),
    ((30, 10), dict(num_disp=16, block=11)),     # width B - 1
    ((30, 11), dict(num_disp=16, block=11, texture_threshold=0)),   # width B
    ((10, 200), dict(num_disp=16, block=11)),    # rows < B
    ((25, 100), dict(num_disp=256, block=5)),    # D > cols
    ((21, 2048), dict(num_disp=64, block=21)),   # the widest this build handles
    ((1, 1), dict()),
])
def test_device_equals_restatement_over_geometries(viso, shape, params):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    L, R = _pair(rng, *shape) if shape[1] > 1 else (rng.integers(0, 256, shape).astype(np.uint8),) * 2
    assert np.array_equal(libviso_amd.stereo_disparity(L, R, **params), DR.disparity(L, R, **params))


def test_largest_cost_on_the_device(viso):
    L, R = largest_cost_pair()
    prm = dict(num_disp=16, block=21, prefilter_cap=63, texture_threshold=0, uniqueness=0, lr_max_diff=-1)
    assert np.array_equal(libviso_amd.stereo_disparity(L, R, **prm), DR.disparity(L, R, **prm))


def test_slanted_plane_accuracy_on_the_device(viso):
    L, R, dtrue = DR.slanted_pair(seed=3)
    d = libviso_amd.stereo_disparity(L, R)
    valid, med, big = DR.accuracy(d, dtrue)
    print(f"device: valid {valid:.3f} median {med:.3f} px > 1 px {big:.4f}")
    assert valid >= 0.85 and med <= 0.12 and big <= 0.01
    f = libviso_amd.disparity_to_float(d)
    assert np.array_equal(np.isnan(f), d == DR.INVALID)


def _seq():
    return synth.make_subpixel_image_sequence(4, 6, n_kp=500, width=640, height=200)


def _run(ctx, seq, disp, seed=3):
    nf, cap = seq["kp"].shape[0], seq["kp"].shape[2]
    b = libviso_amd.Batch(ctx, nf, cap)
    b.upload_images(seq["images"], seq["kp"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=seed)
    b.set_covariance(1)
    b.set_refine(1)
    b.set_window_refine(3)
    if disp is not None:
        b.set_disparity(disp)
    b.run_images()
    return b


def test_batch_equals_direct_and_leaves_the_pipeline_untouched(viso):
    seq = _seq()
    ctx = libviso_amd.Context(0)
    ref = _run(ctx, seq, None)
    prm = dict(num_disp=64, block=9)
    b = _run(ctx, seq, prm)
    nf = seq["kp"].shape[0]
    all_d = b.disparities()
    for t in range(nf):
        want = libviso_amd.stereo_disparity(seq["images"][t, 0], seq["images"][t, 1], **prm)
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
    # matcher_only runs compute it too
    b.set_disparity(num_disp=16, block=5)
    b.run_images(matcher_only=True)
    assert np.array_equal(b.disparity(2), libviso_amd.stereo_disparity(seq["images"][2, 0], seq["images"][2, 1], num_disp=16, block=5))
    with pytest.raises(TypeError):
        b.set_disparity(libviso_amd.disparity_params(), block=5)
    # off: the getters refuse
    b.set_disparity(None)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.disparity(0)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.run_disparity()
    b.close(); ref.close(); ctx.close()


def test_valid_shares_on_the_subpixel_sequence(viso):
    """The shares of valid pixels on the flat noisy background of make_subpixel_image_sequence: defaults 0.48, m = -1 0.55,
    u = 0 and m = -1 0.97, the device equal to the restatement."""
    seq = synth.make_subpixel_image_sequence(2, 2, n_kp=1500)
    L, R = seq["images"][1]
    shares = []
    for p in (dict(), dict(lr_max_diff=-1), dict(uniqueness=0, lr_max_diff=-1)):
        d = libviso_amd.stereo_disparity(L, R, **p)
        assert np.array_equal(d, DR.disparity(L, R, **p))
        shares.append(float((d != DR.INVALID).mean()))
    print("valid shares (defaults, m = -1, u = 0 and m = -1):", shares)
    assert all(abs(s - w) <= 0.02 for s, w in zip(shares, (0.477, 0.548, 0.966))), shares


def test_run_disparity_without_keypoints_and_geometry_growth(viso):
    rng = np.random.default_rng(7)
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 3, 64)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.run_disparity()   # off
    b.set_disparity(num_disp=32, block=7)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.run_disparity()   # no images
    for shape in ((40, 120), (60, 333)):   # the images grow after set_disparity: the maps follow
        imgs = np.stack([np.stack(_pair(rng, *shape)) for _ in range(3)])
        b.upload_images_only(imgs)
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b.disparity(0)   # nothing computed yet for this geometry
        b.run_disparity()
        d = b.disparities()
        assert d.shape == (3,) + shape
        for t in range(3):
            assert np.array_equal(d[t], DR.disparity(imgs[t, 0], imgs[t, 1], num_disp=32, block=7))
    with pytest.raises(libviso_amd.VisoError):
        b.set_disparity(num_disp=20)
    b.close(); ctx.close()


def test_descriptor_in_run_refuses_and_the_batch_stays_usable(viso, oracle):
    seq = synth.make_sequence(4, 4, n_kp=400, width=500, height=200)
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 4, 400)
    b.upload(seq["kp"], seq["desc"], seq["n"])
    b.set_params(st, tm, seq["param"], seed=1)
    b.set_disparity({})
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.run()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.run_matcher()
    b.set_disparity(None)
    b.run()
    tr, ok, n_inl = b.poses()
    want = oracle.sequence(seq["kp"], seq["desc"], seq["n"], st, tm, seq["param"], seed=1)
    assert np.array_equal(ok, want["ok"]) and np.array_equal(n_inl, want["n_inl"])
    b.close(); ctx.close()


def test_rectified_images_are_what_the_kernel_reads(viso):
    calib = synth.raw_stereo_calib(3, raw_shape=(250, 730), out_shape=(200, 640))
    rng = np.random.default_rng(9)
    raw = rng.integers(0, 256, (2, 2) + tuple(calib["raw_shape"])).astype(np.uint8)
    out_shape = tuple(calib["out_shape"])
    maps = [libviso_amd.rectify_map(calib["K"][s], calib["D"][s], calib["R"][s], calib["P"][s], out_shape) for s in range(2)]
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 2, 64)
    b.set_rectify(calib["raw_shape"], out_shape, left=maps[0], right=maps[1])
    b.set_disparity(num_disp=48, block=9)
    b.upload_images_only(raw)
    b.run_disparity()
    for t in range(2):
        want = libviso_amd.stereo_disparity(b.image(t, 0), b.image(t, 1), num_disp=48, block=9)
        assert np.array_equal(b.disparity(t), want)
    b.close(); ctx.close()
