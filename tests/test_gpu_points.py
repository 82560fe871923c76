"""The reprojection of dense maps to 3-D points on the device (include/viso_hip.h, viso_disparity_to_points /
viso_batch_get_disparity_points; points_kernel of libviso_amd/csrc/speckle.hip) against its numpy restatement
(tests/speckle_ref.py), bit for bit, and against the plane the slanted pair was rendered from."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import hostmath, synth
from libviso_amd.abi import MatchParams, Param

import disparity_ref as DR
import speckle_ref as K
from test_speckle_cpu import random_map

pytestmark = pytest.mark.gpu

INV = K.INVALID
POSE = np.linalg.inv(hostmath.tr2mat([0.013, -0.021, 0.007, 0.31, -0.12, 1.47]))   # a rotation and a translation


def _param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)   # non-integer cu, cv


@pytest.mark.parametrize("shape", [(376, 1241), (37, 333), (1, 1), (1, 50), (50, 1), (21, 2048), (15, 63), (16, 64), (17, 65)])
def test_device_equals_restatement(viso, shape):
    rng = np.random.default_rng(shape[0] * 3 + shape[1])
    m = random_map(rng, *shape, spread=2100, invalid=0.2)
    m.flat[0] = 0                          # a disparity of 0 never divides
    m.flat[-1] = 15 if m.size > 1 else 0
    prm = _param()
    for pose in (None, np.eye(4), POSE):
        for md in (1, 16, 160):
            got = libviso_amd.disparity_to_points(m, prm, pose=pose, min_disp16=md)
            assert got.shape == shape + (3,) and got.dtype == np.float32
            assert K.points_equal(got, K.points(m, prm, pose, md)), (shape, md, pose is None)
            assert np.array_equal(np.isfinite(got[..., 2]), (m != INV) & (m >= md))
    assert K.points_equal(libviso_amd.disparity_to_points(m, prm, pose=np.eye(4)), libviso_amd.disparity_to_points(m, prm))
    assert K.points_equal(libviso_amd.disparity_to_points(m, prm, pose=POSE[:3]), libviso_amd.disparity_to_points(m, prm, pose=POSE))


def test_batch_points_equal_the_direct_call(viso):
    seq = synth.make_subpixel_image_sequence(4, 6, n_kp=500, width=640, height=200)
    nf, cap = seq["kp"].shape[0], seq["kp"].shape[2]
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, nf, cap)
    b.upload_images(seq["images"], seq["kp"], seq["n"])
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.disparity_points(0)          # no parameters, no maps
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=3)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.disparity_points(0)          # dense disparity is off
    b.set_disparity(num_disp=64)
    b.set_speckle(max_size=50)
    b.run_images()
    tr, ok, _ = b.poses()
    poses, valid = hostmath.chain_poses(tr, ok)
    assert len(valid) >= 2
    for k, t in enumerate(valid):
        d = b.disparity(t)
        for pose, md in ((None, 1), (poses[k + 1], 1), (poses[k + 1], 32)):
            got = b.disparity_points(t, pose=pose, min_disp16=md)
            assert K.points_equal(got, libviso_amd.disparity_to_points(d, seq["param"], pose=pose, min_disp16=md))
            assert K.points_equal(got, K.points(d, seq["param"], pose, md))
    # the older call of the same family is untouched: the solver's sparse inputs
    X, obs = b.points(valid[0])
    assert X.shape[0] == 3 and obs.shape[0] == 4
    for bad in (dict(t=-1), dict(t=nf), dict(t=0, min_disp16=0)):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b.disparity_points(**bad)
    b.close(); ctx.close()


def test_points_of_the_slanted_pair_lie_on_its_plane(viso):
    """slanted_pair renders a scene whose true disparity dtrue(x, y) is known per pixel, so the plane it was rendered from is
    Z* = f base / dtrue, X* = (x - cu) Z* / f, Y* = (y - cv) Z* / f.  A point's distance from it along its ray, expressed as the
    disparity error that explains it, is e_px = |Z - Z*| d / Z*.

    The bound is derived here, from the error of the unfiltered map against dtrue: err = |d - dtrue| over its n valid pixels.  The
    points come from a subset of those pixels (the filter and min_disp16 only remove, n_r of them), and the kept pixels keep
    their values.  The median of a subset that lost n_r elements is at most the superset's quantile at (n + n_r) / 2n (all removed
    ones below it), and its count beyond 1 px is at most the superset's.  Added: 2^-20 relative for the one rounding of Z to
    float32 (2^-24) and the double arithmetic on both sides."""
    L, R, dtrue = DR.slanted_pair()
    raw = libviso_amd.stereo_disparity(L, R)
    v = raw != INV
    err = np.abs(raw[v] / 16.0 - dtrue[v])
    d16 = libviso_amd.filter_speckles(raw)
    prm = _param()
    P = libviso_amd.disparity_to_points(d16, prm, min_disp16=16)
    fin = np.isfinite(P[..., 2])
    assert np.array_equal(fin, (d16 != INV) & (d16 >= 16)) and not (fin & ~v).any() and fin.mean() > 0.9
    n, n_r = int(v.sum()), int(v.sum() - fin.sum())
    med_bound = float(np.quantile(err, min(1.0, (n + n_r) / (2.0 * n)), method="higher"))
    big_bound = float((err > 1.0).sum()) / float(fin.sum())
    d = d16[fin] / 16.0
    zs = prm.f * prm.base / dtrue[fin]
    z = P[..., 2][fin].astype(np.float64)
    slack = 2.0 ** -20 * d
    e_px = np.abs(z - zs) * d / zs
    med, big = float(np.median(e_px)), float((e_px > 1.0 + slack).mean())
    print(f"unfiltered map: median {float(np.median(err)):.4f} px, {n_r} of {n} pixels removed; bounds: median {med_bound:.4f} px, "
          f"beyond 1 px {big_bound:.5f}; points: median {med:.4f} px, beyond 1 px {big:.5f}")
    assert med <= med_bound + float(slack.max()) and big <= big_bound
    # X and Y: the point is on its pixel's ray, so its distance from the plane's point is the depth error along that ray
    yy, xx = np.nonzero(fin)
    xs, ys = (xx - prm.cu) * zs / prm.f, (yy - prm.cv) * zs / prm.f
    assert (np.abs(P[..., 0][fin] - xs) <= np.abs(xs) * (e_px + slack) / d * (1 + 1e-6) + 1e-6).all()
    assert (np.abs(P[..., 1][fin] - ys) <= np.abs(ys) * (e_px + slack) / d * (1 + 1e-6) + 1e-6).all()
