"""The opt-in motion covariance on the device (include/viso_hip.h, "motion covariance"; libviso_amd/csrc/covariance.hip) against
its numpy restatement (tests/covariance_ref.py): the direct call, the batch paths, invariance of everything else, chunking, and
statistical consistency on a noisy synthetic sequence."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MatchParams, Param

import covariance_ref as CR
from estimator_util import seq_batch

pytestmark = pytest.mark.gpu

FIELDS = ("cov", "delta", "sigma2", "gap")


def _check(got, want, what):
    assert int(got["status"]) == want["status"] and int(got["n"]) == want["n"], (what, int(got["status"]), want["status"])
    for k in FIELDS:
        assert np.all(np.isfinite(got[k])), (what, k)
    if want["status"] != 1:
        for k in FIELDS:
            assert not np.any(got[k]), (what, k)
        return
    S_ref, S = want["cov"], np.asarray(got["cov"])
    assert np.array_equal(S, S.T), what
    assert CR.whitened_error(S_ref, S) <= 1e-9, (what, CR.whitened_error(S_ref, S))
    Wi = np.linalg.inv(S_ref)
    dd = np.asarray(got["delta"]) - want["delta"]
    scale = max(1.0, float(np.sqrt(want["delta"] @ Wi @ want["delta"])))
    assert np.sqrt(dd @ Wi @ dd) <= 1e-9 * scale, what
    assert abs(float(got["sigma2"]) - want["sigma2"]) <= 1e-9 * want["sigma2"], what
    assert abs(float(got["gap"]) - want["gap"]) <= 1e-9 * max(1.0, want["gap"]), what


def test_direct_call_against_the_restatement(viso):
    for m in (6, 7, 40, 300, 1200, 3000):
        X, obs, tr_true, param = synth.make_solver_case(m, m=m, outlier_frac=0.0 if m < 40 else 0.2)
        if m >= 40:
            r, tr, inl = libviso_amd.ransac_minimize_reproj(X, obs, param, seed=1, frame=m)
            assert r == 1 and len(inl) >= 6
        else:
            tr, inl = tr_true, np.arange(m, dtype=np.int32)
        for mode, sigma in ((1, None), (2, 0.3), (2, 1.7)):
            got = libviso_amd.pose_covariance(X, obs, tr, inl, param, mode=mode, sigma=sigma)
            want = CR.motion_cov(X, obs, tr, inl, param, mode, sigma)
            assert want["status"] == 1
            _check(got, want, (m, mode))
            again = libviso_amd.pose_covariance(X, obs, tr, inl, param, mode=mode, sigma=sigma)
            assert got.tobytes() == again.tobytes()


def test_direct_call_degenerate_cases(viso):
    X, obs, tr, param = synth.make_solver_case(2, m=50, outlier_frac=0.0)
    cases = []
    cases.append((X, obs, np.arange(5, dtype=np.int32), -1))                          # n < 6
    cases.append((X, obs, np.zeros(0, np.int32), -1))
    Xd = np.repeat(X[:, :1], 50, axis=1)                                               # one point, 50 times
    od = np.repeat(obs[:, :1], 50, axis=1)
    cases.append((Xd, od, np.arange(50, dtype=np.int32), -2))
    ray = X[:, :1] / X[2, 0] * np.linspace(6.0, 40.0, 50)[None, :]                   # collinear on one ray of the previous camera
    R, t = synth.rot_from_tr(tr)
    Xc = R @ ray + t[:, None]
    f, cu, cv, b = param.f, param.cu, param.cv, param.base
    orr = np.stack([f * Xc[0] / Xc[2] + cu, f * Xc[1] / Xc[2] + cv, f * (Xc[0] - b) / Xc[2] + cu, f * Xc[1] / Xc[2] + cv])
    cases.append((ray, orr, np.arange(50, dtype=np.int32), -2))
    for i, (XX, oo, inl, status) in enumerate(cases):
        for mode, sigma in ((1, None), (2, 0.5)):
            got = libviso_amd.pose_covariance(XX, oo, tr, inl, param, mode=mode, sigma=sigma)
            want = CR.motion_cov(XX, oo, tr, inl, param, mode, sigma)
            assert want["status"] == status, i
            _check(got, want, (i, mode))


def _check_batch_frames(b, param, mode, sigma=None):
    recs = b.covariances()
    n_valid = 0
    assert recs[0]["status"] == 0 and not recs[0]["cov"].any()
    for t in range(1, b.nf):
        X, obs = b.points(t)
        ok, tr, inl = b.pose(t)
        want = CR.motion_cov(X, obs, tr, inl, param, mode, sigma, ok=ok)
        _check(recs[t], want, t)
        assert recs[t].tobytes() == b.covariance(t).tobytes()
        if ok:
            direct = libviso_amd.pose_covariance(X, obs, tr, inl, param, mode=mode, sigma=sigma)
            assert direct.tobytes() == recs[t].tobytes(), t
        n_valid += int(recs[t]["status"]) == 1
    return n_valid


@pytest.fixture(scope="module")
def seq33():
    return synth.make_sequence(21, 33, n_kp=1500)


def test_batch_path_against_restatement_and_direct_call(viso, seq33):
    ctx = libviso_amd.Context(0)
    for mode, sigma in ((1, None), (2, 0.4)):
        b = seq_batch(ctx, seq33, cov=(mode, sigma))
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
    b.set_covariance(1)
    b.run_images()
    assert _check_batch_frames(b, seq["param"], 1) >= 10
    b.run_images(matcher_only=True)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.covariances()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.covariance(3)
    b.run_images()                     # usable again
    assert b.covariances()["status"][1:].max() == 1
    b.close(); ctx.close()


def test_mode0_and_mode1_runs_are_otherwise_identical(viso, seq33):
    ctx = libviso_amd.Context(0)
    b0 = seq_batch(ctx, seq33, cov=(0,))
    b1 = seq_batch(ctx, seq33, cov=(1,))
    for a, c in zip(b0.poses(), b1.poses()):
        assert a.tobytes() == c.tobytes()
    for t in range(b0.nf):
        p0, p1 = b0.pose(t), b1.pose(t)
        assert p0[0] == p1[0] and p0[1].tobytes() == p1[1].tobytes() and p0[2].tobytes() == p1[2].tobytes()
    for a, c in zip(b0.hypotheses(), b1.hypotheses()):
        assert np.asarray(a).tobytes() == np.asarray(c).tobytes()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b0.covariances()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b0.covariance(1)
    # the same batch: on, then off again -- a mode-0 run leaves no records behind
    b1.set_covariance(0)
    b1.run()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b1.covariances()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b1.set_covariance(2, -1.0)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b1.set_covariance(3)
    b1.set_covariance(1)
    b1.run()
    assert b1.covariances()["status"][1:].max() == 1
    b0.close(); b1.close(); ctx.close()


def test_chunked_batches_give_byte_equal_records(viso):
    seq = synth.make_sequence(7, 64, n_kp=1200)
    ctx = libviso_amd.Context(0)
    whole = seq_batch(ctx, seq, cov=(1,)).covariances()
    a = seq_batch(ctx, seq, cov=(1,), frames=slice(0, 32)).covariances()
    c = seq_batch(ctx, seq, cov=(1,), first=31, frames=slice(31, 64)).covariances()   # frame 31 is the second chunk's halo
    assert a[1:].tobytes() == whole[1:32].tobytes()
    assert c[0]["status"] == 0
    assert c[1:].tobytes() == whole[32:].tobytes()
    assert (whole["status"][1:] == 1).sum() >= 60
    ctx.close()


def test_consistency_on_a_noisy_sequence(viso):
    sigma = 0.3
    seq = synth.make_noisy_sequence(17, 257, sigma)
    ctx = libviso_amd.Context(0)
    out = {}
    for mode, s in ((2, sigma), (1, None)):
        b = seq_batch(ctx, seq, cov=(mode, s))
        recs = b.covariances()
        tr, ok, _n = b.poses()
        good = np.nonzero(recs["status"] == 1)[0]
        nees = []
        for t in good:
            e = tr[t] + recs[t]["delta"] - seq["tr_gt"][t]
            nees.append(e @ np.linalg.solve(recs[t]["cov"], e))
        out[mode] = (float(np.mean(nees)), float(np.mean(recs["gap"][good] > 16.8)), len(good),
                     float(np.median(recs["sigma2"][good])))
        b.close()
    ctx.close()
    print(f"\nmode 2: mean NEES {out[2][0]:.3f}, gap > 16.8 in {100 * out[2][1]:.1f} % of {out[2][2]} frames")
    print(f"mode 1: mean NEES {out[1][0]:.3f}, median sigma2 {out[1][3]:.4f} (true {sigma ** 2:.4f})")
    assert out[2][2] >= 250
    assert 5.0 <= out[2][0] <= 7.2
    assert 4.5 <= out[1][0] <= 8.0


def _parse_cov_file(data):
    rows = [line.split() for line in data.decode().splitlines()]
    return [(int(r[0]), int(r[1]), float(r[2]), float(r[3]), [float(v) for v in r[4:]]) for r in rows]


def test_kitti_runners_with_covariance(viso, tmp_path):
    """viso_kitti --covariance and kitti_shard --covariance: byte-identical files for W = 1, 2, 3, chunk sizes and partitions
    (a chunk's halo frame is recomputed like any other), equal to Batch.covariances() on the same frames; pose files unchanged."""
    import os
    import subprocess
    import sys

    import kitti_tree
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    home, first, nf = str(tmp_path), 4, 12
    seq = synth.make_subpixel_image_sequence(31, nf, n_kp=1500, width=720, height=240)
    kitti_tree.write_tree(home, "07", seq, first_index=first)
    env = dict(os.environ, KITTI_HOME=home, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(cmd, sha, cov):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert r.returncode == 0, r.stdout + r.stderr
        poses = open(os.path.join(home, "results", "07", sha, "data", "07.txt"), "rb").read()
        return poses, open(cov, "rb").read()

    plain = subprocess.run([exe, "p0", "07", str(first)], capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    poses0 = open(os.path.join(home, "results", "07", "p0", "data", "07.txt"), "rb").read()
    files = {}
    for extra, tag in (([], "m1"), (["--covariance-sigma", "0.5"], "m2")):
        outs = []
        for w, chunk in ((1, 64), (2, 64), (3, 3), (1, 4)):
            cov = os.path.join(home, f"{tag}_k{w}_{chunk}.txt")
            cmd = [exe, f"{tag}k{w}{chunk}", "07", str(first), "--covariance", cov, "--chunk", str(chunk)] + extra
            if w > 1:
                cmd += ["--gpus", str(w), "--same-device"]
            outs.append(run(cmd, f"{tag}k{w}{chunk}", cov))
        for w in (1, 2, 3):
            cov = os.path.join(home, f"{tag}_s{w}.txt")
            outs.append(run([sys.executable, "-m", "libviso_amd.kitti_shard", f"{tag}s{w}", "07", str(first), "--gpus", str(w),
                             "--backend", "gloo", "--same-device", "--covariance", cov] + extra, f"{tag}s{w}", cov))
        for poses, data in outs:
            assert poses == poses0                     # pose files are unchanged by the option
            assert data == outs[0][1]
        files[tag] = outs[0][1]
    assert files["m1"] != files["m2"]
    bad = subprocess.run([exe, "bad", "07", str(first), "--covariance-sigma", "0.5"], capture_output=True, text=True, timeout=60,
                         env=env, cwd=root)
    assert bad.returncode != 0                         # --covariance-sigma needs --covariance

    # the batch API on the same frames: Harris 1200 / 24 x 5, RANSAC keyed by the frame index
    P1, P2 = seq["P1"], seq["P2"]
    param = Param.default(base=abs(P2[0, 3] / P2[0, 0]), f=P1[0, 0], cu=P1[0, 2], cv=P1[1, 2])
    ctx = libviso_amd.Context(0)
    for tag, mode, sigma in (("m1", 1, None), ("m2", 2, 0.5)):
        b = libviso_amd.Batch(ctx, nf, 1200)
        b.upload_images_only(seq["images"])
        b.detect(n_features=1200, nbinx=24, nbiny=5)
        b.set_params(MatchParams.stereo(libviso_amd.F_from_P(P1, P2)), MatchParams.temporal(), param, seed=0, first_frame=first)
        b.set_covariance(mode, sigma)
        b.run_images()
        recs = b.covariances()
        lines = _parse_cov_file(files[tag])
        assert len(lines) == nf - 1
        iu = np.triu_indices(6)
        for t in range(1, nf):
            st, n, s2, gap, upper = lines[t - 1]
            c = recs[t]
            assert (st, n) == (int(c["status"]), int(c["n"])), t
            assert s2 == float(c["sigma2"]) and gap == float(c["gap"]) and upper == [float(v) for v in c["cov"][iu]], t
        assert (recs["status"][1:] == 1).sum() >= nf - 3
        b.close()
    ctx.close()
