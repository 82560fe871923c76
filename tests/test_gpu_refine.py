"""The opt-in two-frame bundle adjustment on the device (include/viso_hip.h, "motion refinement"; libviso_amd/csrc/refine.hip)
against its numpy restatement (tests/refine_ref.py): the direct call, degenerate inputs, the batch paths, invariance of everything
else, chunking, and accuracy and consistency on a noisy synthetic sequence."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MatchParams

import covariance_ref as CR
import refine_ref as RR
from estimator_util import TR_WHITE, bound, check_gap, check_iters, check_points, note_gap, seq_batch, tr_abs_limits

pytestmark = pytest.mark.gpu

ZERO_FIELDS = ("cov", "sigma2", "cost0", "cost", "gap", "iters")


def _check(got, want, what, far=False):
    assert int(got["status"]) == want["status"] and int(got["n"]) == want["n"], (what, int(got["status"]), want["status"])
    for k in ("tr",) + ZERO_FIELDS:
        assert np.all(np.isfinite(got[k])), (what, k)
    if want["status"] != 1:
        assert np.asarray(got["tr"]).tobytes() == np.asarray(want["tr"]).tobytes(), what
        for k in ZERO_FIELDS:
            assert not np.any(got[k]), (what, k)
        return
    check_iters(got["iters"], want, what)
    d = np.asarray(got["tr"]) - want["tr"]
    # in units of the estimate's own standard deviation.  The stop test (C_old - C_new <= 1e-12 C_old) leaves the two summation
    # orders free to end a rounding-level accepted step or two apart: the bound is the strict one plus 4 x the restatement's own
    # last steps (estimator_util.bound), per case
    white = float(np.sqrt(d @ np.linalg.solve(want["cov"] / max(want["sigma2"], 1e-300), d) / max(want["sigma2"], 1e-300)))
    white_max = bound(TR_WHITE, want["slack"]["tr_white"])
    abs_max = bound(tr_abs_limits(want["n"]), want["slack"]["tr_abs"])
    note_gap("refine tr whitened", white, white_max, what)
    note_gap("refine tr absolute", float(np.abs(d).max()), abs_max, what)
    if want["n"] >= 40:
        assert white <= white_max, (what, white, want["slack"]["tr_white"], d)
    assert np.abs(d).max() <= abs_max, (what, np.abs(d).max(), want["slack"]["tr_abs"])
    S = np.asarray(got["cov"])
    assert np.array_equal(S, S.T), what
    assert CR.whitened_error(want["cov"], S) <= 1e-7, (what, CR.whitened_error(want["cov"], S))
    for k in ("sigma2", "cost0", "cost"):
        assert abs(float(got[k]) - want[k]) <= 1e-9 * max(want[k], 1e-300), (what, k, float(got[k]), want[k])
    check_gap(float(got["gap"]), want, what, far)


def test_direct_call_against_the_restatement(viso):
    for m in (6, 7, 40, 300, 1200, 3000):
        X, obs, tr_true, param = synth.make_solver_case(m, m=m, outlier_frac=0.0 if m < 40 else 0.2)
        if m >= 40:
            r, tr, inl = libviso_amd.ransac_minimize_reproj(X, obs, param, seed=1, frame=m)
            assert r == 1 and len(inl) >= 6
        else:
            tr, inl = tr_true, np.arange(m, dtype=np.int32)
        for mode, sigma in ((1, None), (2, 0.3)):
            got, pts = libviso_amd.pose_refine(X, obs, tr, inl, param, mode=mode, sigma=sigma)
            want = RR.refine(X, obs, tr, inl, param, mode, sigma)
            assert want["status"] == 1, m
            _check(got, want, (m, mode))
            assert pts.shape == (3, want["n"])
            check_points(pts, want, (m, mode))
            again, pts2 = libviso_amd.pose_refine(X, obs, tr, inl, param, mode=mode, sigma=sigma)
            assert got.tobytes() == again.tobytes() and pts.tobytes() == pts2.tobytes()


def test_direct_call_degenerate_inputs(viso):
    X, obs, tr, param = synth.make_solver_case(2, m=50, outlier_frac=0.0)
    inl = np.arange(50, dtype=np.int32)
    cases = []
    for n_keep in (5, 6, 7):                                  # n = 5, 6, 7 after dropping bad points from L
        Xb = X.copy()
        drop = np.arange(n_keep, 50)
        Xb[2, drop[0::3]] = -Xb[2, drop[0::3]]                # Z < 0
        Xb[2, drop[1::3]] = 0.0                               # Z = 0
        Xb[0, drop[2::3]] = np.inf                            # not finite
        cases.append((Xb, obs, inl[::-1].copy(), -1 if n_keep < 6 else 1))
    Xn = X.copy()
    Xn[1, 3] = np.nan
    cases.append((Xn, obs, inl, 1))
    cases.append((np.repeat(X[:, :1], 50, axis=1), np.repeat(obs[:, :1], 50, axis=1), inl, -2))   # one point, 50 times
    Xh = X.copy()
    Xh[2, 7] = 1e-306                                         # finite with Z > 0, but f X / Z overflows: the cost is not finite
    cases.append((Xh, obs, inl, -3))
    for i, (XX, oo, ll, status) in enumerate(cases):
        for mode, sigma in ((1, None), (2, 0.5)):
            got, pts = libviso_amd.pose_refine(XX, oo, tr, ll, param, mode=mode, sigma=sigma)
            want = RR.refine(XX, oo, tr, ll, param, mode, sigma)
            assert want["status"] == status, (i, want["status"])
            _check(got, want, (i, mode))
            if status == 1:
                check_points(pts, want, (i, mode))


def _check_batch_frames(b, param, mode, sigma=None):
    recs = b.refines()
    n_valid = 0
    assert recs[0]["status"] == 0 and not recs[0]["cov"].any()
    for t in range(1, b.nf):
        X, obs = b.points(t)
        ok, tr, inl = b.pose(t)
        want = RR.refine(X, obs, tr, inl, param, mode, sigma, ok=ok)
        _check(recs[t], want, t)
        assert recs[t].tobytes() == b.refine(t).tobytes()
        idx, pts = b.refined_points(t)
        if ok:
            direct, dpts = libviso_amd.pose_refine(X, obs, tr, inl, param, mode=mode, sigma=sigma)
            assert direct.tobytes() == recs[t].tobytes(), t
            assert dpts.tobytes() == pts.tobytes(), t
        if int(recs[t]["status"]) == 1:
            assert np.array_equal(idx, want["idx"])
            check_points(pts, want, t)
        else:
            assert len(idx) == 0 and pts.shape == (3, 0)
        n_valid += int(recs[t]["status"]) == 1
    return n_valid


@pytest.fixture(scope="module")
def seq33():
    return synth.make_sequence(21, 33, n_kp=1500)


def test_batch_path_against_restatement_and_direct_call(viso, seq33):
    ctx = libviso_amd.Context(0)
    for mode, sigma in ((1, None), (2, 0.4)):
        b = seq_batch(ctx, seq33, refine=(mode, sigma))
        assert _check_batch_frames(b, seq33["param"], mode, sigma) >= 30
        b.close()
    ctx.close()


@pytest.mark.parametrize("subpixel", [0, 1])
def test_image_in_batch_path(viso, subpixel):
    seq = synth.make_subpixel_image_sequence(8, 16, n_kp=600, width=640, height=200)
    ctx = libviso_amd.Context(0)
    nf, cap = seq["kp"].shape[0], seq["kp"].shape[2]
    b = libviso_amd.Batch(ctx, nf, cap)
    b.upload_images(seq["images"], seq["kp"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=5)
    b.set_subpixel(subpixel)
    b.set_refine(1)
    b.run_images()
    assert _check_batch_frames(b, seq["param"], 1) >= 10
    b.run_images(matcher_only=True)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.refines()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.refine(3)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.refined_points(3)
    b.run_images()                     # usable again
    assert b.refines()["status"][1:].max() == 1
    b.close(); ctx.close()


def test_refine_on_and_off_leave_everything_else_identical(viso, seq33):
    ctx = libviso_amd.Context(0)
    b0 = seq_batch(ctx, seq33, cov=(1,), refine=(0,))
    b1 = seq_batch(ctx, seq33, cov=(1,), refine=(1,))
    for a, c in zip(b0.poses(), b1.poses()):
        assert a.tobytes() == c.tobytes()
    for t in range(b0.nf):
        p0, p1 = b0.pose(t), b1.pose(t)
        assert p0[0] == p1[0] and p0[1].tobytes() == p1[1].tobytes() and p0[2].tobytes() == p1[2].tobytes()
    assert b0.covariances().tobytes() == b1.covariances().tobytes()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b0.refines()
    b1.set_refine(0)
    b1.run()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b1.refines()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b1.set_refine(2, -1.0)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b1.set_refine(3)
    b1.set_refine(1)
    b1.run()
    assert b1.refines()["status"][1:].max() == 1
    b0.close(); b1.close(); ctx.close()


def test_chunked_batches_give_byte_equal_records(viso):
    seq = synth.make_sequence(7, 64, n_kp=1200)
    ctx = libviso_amd.Context(0)
    bw = seq_batch(ctx, seq, refine=(1,))
    whole = bw.refines()
    ba = seq_batch(ctx, seq, refine=(1,), frames=slice(0, 32))
    bc = seq_batch(ctx, seq, refine=(1,), first=31, frames=slice(31, 64))   # frame 31 is the second chunk's halo
    a, c = ba.refines(), bc.refines()
    assert a[1:].tobytes() == whole[1:32].tobytes()
    assert c[0]["status"] == 0
    assert c[1:].tobytes() == whole[32:].tobytes()
    for t in (5, 40):
        got = ba.refined_points(t) if t < 32 else bc.refined_points(t - 31)
        want = bw.refined_points(t)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    assert (whole["status"][1:] == 1).sum() >= 60
    ctx.close()


def test_accuracy_and_consistency_on_a_noisy_sequence(viso):
    sigma = 0.3
    seq = synth.make_noisy_sequence(17, 257, sigma)
    gt = seq["tr_gt"]
    ctx = libviso_amd.Context(0)
    b = seq_batch(ctx, seq, refine=(2, sigma))
    recs = b.refines()
    tr, ok, _n = b.poses()
    good = np.nonzero(recs["status"] == 1)[0]
    assert len(good) >= 250
    e_ref, e_ba = tr[good] - gt[good], recs["tr"][good] - gt[good]
    rot = (np.median(np.linalg.norm(e_ref[:, :3], axis=1)), np.median(np.linalg.norm(e_ba[:, :3], axis=1)))
    tra = (np.median(np.linalg.norm(e_ref[:, 3:], axis=1)), np.median(np.linalg.norm(e_ba[:, 3:], axis=1)))
    nees = [e @ np.linalg.solve(recs[t]["cov"], e) for t, e in zip(good, e_ba)]
    it = recs["iters"][good]
    print(f"\nmedian rotation error {rot[0]:.3e} -> {rot[1]:.3e} rad, translation {tra[0]:.3e} -> {tra[1]:.3e}; "
          f"mean NEES {np.mean(nees):.3f}; iterations mean {it.mean():.2f} max {it.max()}")
    assert rot[1] < 0.8 * rot[0] and tra[1] < 0.8 * tra[0]
    assert 5.0 <= float(np.mean(nees)) <= 7.2
    assert np.all(recs["gap"][good] < 1e-3)
    # mode 1 on the same run: sigma^2 estimates the truth
    b.set_refine(1)
    b.run()
    r1 = b.refines()
    g1 = r1["status"] == 1
    assert abs(np.median(r1["sigma2"][g1]) - sigma ** 2) < 0.1 * sigma ** 2
    assert np.array_equal(r1["tr"], recs["tr"])      # the mode changes sigma^2, not the path
    b.close(); ctx.close()
