"""No-GPU checks of the opt-in motion covariance (include/viso_hip.h, "motion covariance"): the definition against numeric
derivatives of the fully converged weighted least squares, its statistical consistency (Monte Carlo, numpy), the host-only
trajectory propagation (viso_chain_covariances) against its restatement (tests/covariance_ref.py), argument errors, and the
device entry points failing loudly without a device."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MOTION_COV_DTYPE, Param

import covariance_ref as CR


def _project(X, tr, param):
    return CR.predict(X, tr, param)[0]


def _scene(rng, m, zmin=5.0, zmax=50.0):
    """True previous-frame points (3, m) in view of both frames, a motion, and their exact observations in both frames."""
    f, cu, cv, b = synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV, synth.KITTI_BASE
    param = Param.default(base=b, f=f, cu=cu, cv=cv)
    tr = np.concatenate([rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.05, 0.05, 2), -rng.uniform(0.5, 1.5, 1)])
    X = synth._new_points(rng, m, 1241, 376, zmin, zmax, f, cu, cv).T.copy()
    xp = _project(X, np.zeros(6), param)
    xc = _project(X, tr, param)
    return X, xp, xc, tr, param


def test_sandwich_equals_numeric_derivative_of_the_converged_wls():
    rng = np.random.default_rng(3)
    for rep in range(3):
        X, xp, xc, tr, param = _scene(rng, 40)
        inl = np.arange(X.shape[1])
        Xt = CR.triangulate(xp, param)
        rec = CR.motion_cov(Xt, xc, tr, inl, param, mode=2, sigma=1.0)
        assert rec["status"] == 1
        # noise-free observations: the optimum is tr itself, and the weights' own dependence on uL enters only through r = 0
        assert np.abs(CR.wls(Xt, xc, inl, param, tr) - tr).max() < 1e-12
        h = 1e-4
        Dc = np.zeros((6, xc.size))
        Dp = np.zeros((6, xp.size))
        for which, x, D in (("c", xc, Dc), ("p", xp, Dp)):
            for i in range(x.size):
                e = np.zeros(x.size)
                e[i] = h
                outs = []
                for s in (1, -1):
                    xx = x + s * e.reshape(x.shape)
                    if which == "c":
                        outs.append(CR.wls(Xt, xx, inl, param, tr))
                    else:
                        outs.append(CR.wls(CR.triangulate(xx, param), xc, inl, param, tr))
                D[:, i] = (outs[0] - outs[1]) / (2 * h)
        num = Dc @ Dc.T + Dp @ Dp.T
        assert not Dp[:, 3 * X.shape[1]:].any()   # vR of the previous frame is not used by triangulation
        assert CR.whitened_error(num, rec["cov"]) < 1e-5, rep
        assert np.linalg.norm(rec["cov"] - num) / np.linalg.norm(num) < 1e-5, rep


def test_monte_carlo_nees_of_the_wls_optimum():
    """2,000 noisy draws, noise in both frames: the mean NEES of the WLS optimum against the truth is 6 within its spread; the model
    without the triangulation term (M = 0) is recorded beside it."""
    rng = np.random.default_rng(11)
    sigma = 0.3
    nees, nees_noM = [], []
    for _ in range(2000):
        X, xp, xc, tr, param = _scene(rng, 60)
        xpn = xp + rng.normal(0, sigma, xp.shape)
        xcn = xc + rng.normal(0, sigma, xc.shape)
        Xt = CR.triangulate(xpn, param)
        inl = np.arange(X.shape[1])
        opt = CR.wls(Xt, xcn, inl, param, tr)
        e = opt - tr
        rec = CR.motion_cov(Xt, xcn, opt, inl, param, mode=2, sigma=sigma)
        rec0 = CR.motion_cov(Xt, xcn, opt, inl, param, mode=2, sigma=sigma, with_M=False)
        assert rec["status"] == 1 and rec0["status"] == 1
        assert np.abs(rec["delta"]).max() < 1e-10   # at the optimum
        nees.append(e @ np.linalg.solve(rec["cov"], e))
        nees_noM.append(e @ np.linalg.solve(rec0["cov"], e))
    mean, mean0 = float(np.mean(nees)), float(np.mean(nees_noM))
    print(f"mean NEES {mean:.3f} (model without the triangulation term: {mean0:.3f})")
    assert 5.6 <= mean <= 6.4
    assert mean0 > 6.4   # the current frame's noise alone does not explain the spread


def _random_records(rng, n, bad=()):
    recs = np.zeros(n, MOTION_COV_DTYPE)
    for t in range(n):
        Q = rng.normal(size=(6, 6)) * np.array([1e-3] * 3 + [1e-2] * 3)
        recs[t]["cov"] = Q @ Q.T
        recs[t]["status"] = 1
    for t in bad:
        recs[t]["status"] = -1
        recs[t]["cov"] = 0
    return recs


def test_chain_matches_the_restatement():
    rng = np.random.default_rng(5)
    n = 40
    tr = np.concatenate([rng.uniform(-0.05, 0.05, (n, 3)), rng.uniform(-0.3, 0.3, (n, 2)), rng.uniform(-1.5, 0.5, (n, 1))], 1)
    for ok, bad in ((np.ones(n, np.int32), ()), ((rng.uniform(size=n) > 0.2).astype(np.int32), ()),
                    ((rng.uniform(size=n) > 0.2).astype(np.int32), (25,))):
        ok[0] = 0
        for t in bad:
            ok[t] = 1   # a chained frame: the chain turns invalid there
        recs = _random_records(rng, n, bad)
        S, valid = libviso_amd.chain_covariances(tr, ok, recs)
        S_ref, valid_ref = CR.chain(tr, ok, recs)
        assert S.shape == S_ref.shape and len(S) == 1 + int(ok.astype(bool).sum())
        assert np.array_equal(valid, valid_ref)
        for k in range(len(S)):
            scale = max(np.abs(S_ref[k]).max(), 1e-300)
            assert np.abs(S[k] - S_ref[k]).max() <= 1e-12 * scale, k
            assert np.array_equal(S[k], S[k].T)
        if bad:
            first = 1 + int(ok[:bad[0]].astype(bool).sum())   # the entry of the bad frame
            assert valid[first] == 0 and not valid[first:].any() and valid[:first].all()
            assert not S[first:].any() and S[first - 1].any()
        else:
            assert valid.all()
    # the list is hostmath.chain_poses' (default, no aliasing quirk)
    poses, vl = libviso_amd.hostmath.chain_poses(tr, ok)
    assert len(poses) == len(S)


def test_G_against_central_differences():
    rng = np.random.default_rng(9)
    for _ in range(20):
        tr = np.concatenate([rng.uniform(-0.3, 0.3, 3), rng.uniform(-2, 2, 3)])
        Ga, Gn = CR.G_analytic(tr), CR.G_numeric(tr)
        assert np.abs(Ga - Gn).max() < 1e-6


def test_two_step_chain_against_numeric_propagation():
    """S_2 against the linearised propagation built from nothing but the chain's definition: xi = Log(P^^-1 P) with
    P = inv(T(tr1)) inv(T(tr2)), its central-difference Jacobian D over (tr1, tr2), S = D diag(cov1, cov2) D'.  Pins the Ad
    transport independently of the form library and restatement share."""
    rng = np.random.default_rng(17)
    tr = np.array([[0] * 6, [0.03, -0.2, 0.1, 0.4, -0.1, -1.2], [-0.05, 0.12, 0.07, -0.3, 0.2, -0.9]], np.float64)
    recs = _random_records(rng, 3)
    S, valid = libviso_amd.chain_covariances(tr, [0, 1, 1], recs)
    inv, T = np.linalg.inv, libviso_amd.hostmath.tr2mat
    P_hat = inv(T(tr[1])) @ inv(T(tr[2]))

    def xi(x):
        return CR.se3_log(inv(P_hat) @ inv(T(x[:6])) @ inv(T(x[6:])))

    x0, h = np.concatenate([tr[1], tr[2]]), 1e-6
    D = np.zeros((6, 12))
    for i in range(12):
        e = np.zeros(12)
        e[i] = h
        D[:, i] = (xi(x0 + e) - xi(x0 - e)) / (2 * h)
    C12 = np.zeros((12, 12))
    C12[:6, :6], C12[6:, 6:] = recs[1]["cov"], recs[2]["cov"]
    want = D @ C12 @ D.T
    assert valid.tolist() == [1, 1, 1]
    assert np.abs(S[2] - want).max() < 1e-6 * np.abs(want).max()


def test_chain_one_step_uses_G():
    """One chained frame: S_1 = G cov G' (S_0 = 0) -- ties the library's G to the restated one entry by entry."""
    rng = np.random.default_rng(13)
    tr = np.array([[0] * 6, [0.03, -0.2, 0.1, 0.4, -0.1, -1.2]], np.float64)
    recs = _random_records(rng, 2)
    S, valid = libviso_amd.chain_covariances(tr, [0, 1], recs)
    G = CR.G_numeric(tr[1])
    want = G @ recs[1]["cov"] @ G.T
    assert valid.tolist() == [1, 1]
    assert np.abs(S[1] - want).max() < 1e-6 * np.abs(want).max()


def test_argument_errors_return_codes():
    L = libviso_amd.load()
    X, obs, tr, param = synth.make_solver_case(1, m=20, outlier_frac=0.0)
    inl = np.arange(20)
    for mode, sigma in ((0, None), (3, None), (-1, None), (2, None), (2, 0.0), (2, -1.0), (2, float("nan")), (2, float("inf"))):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.pose_covariance(X, obs, tr, inl, param, mode=mode, sigma=sigma)
    for bad in (np.array([0, 1, 20]), np.array([-1, 2, 3]), np.arange(21) % 20):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.pose_covariance(X, obs, tr, bad, param, mode=1)
    for Xb, ob in ((X, obs[:, :19]), (X.T, obs), (X, obs[:3]), (X[:2], obs)):   # shapes other than X (3, m), obs (4, m)
        with pytest.raises(ValueError):
            libviso_amd.pose_covariance(Xb, ob, tr, inl[:5], param, mode=1)
    buf = np.zeros(4, MOTION_COV_DTYPE)
    assert L.viso_batch_set_covariance(None, 1, 0.0) == -1
    assert L.viso_batch_get_covariance(None, 0, buf.ctypes.data) == -1
    assert L.viso_batch_get_covariances(None, buf.ctypes.data) == -1
    m = C.c_int(0)
    assert L.viso_batch_get_points(None, 0, None, None, C.byref(m)) == -1
    f64 = C.POINTER(C.c_double)
    i32 = C.POINTER(C.c_int32)
    trs = np.zeros((4, 6))
    ok = np.ones(4, np.int32)
    out = np.zeros((5, 36))
    valid = np.zeros(5, np.int32)
    args = [trs.ctypes.data_as(f64), ok.ctypes.data_as(i32), buf.ctypes.data, 4, out.ctypes.data_as(f64), valid.ctypes.data_as(i32),
            C.byref(m)]
    assert L.viso_chain_covariances(*args) == 1 and m.value == 5
    for i in (0, 1, 2, 4, 5, 6):
        a = list(args)
        a[i] = None
        assert L.viso_chain_covariances(*a) == -1, i
    a = list(args)
    a[3] = -1
    assert L.viso_chain_covariances(*a) == -1
    with pytest.raises(ValueError):
        libviso_amd.chain_covariances(trs, ok[:3], buf)


def test_version_names_the_feature():
    assert b"0.4" in libviso_amd.load().viso_version()


def test_device_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    X, obs, tr, param = synth.make_solver_case(1, m=20, outlier_frac=0.0)
    with pytest.raises(libviso_amd.VisoError, match="-2"):
        libviso_amd.pose_covariance(X, obs, tr, np.arange(20), param, mode=1)


def test_runner_covariance_file_and_options(tmp_path):
    """The runners' covariance file (viso_kitti_write_covariances, the one writer both runners use) and the option checks of
    viso_kitti_set_covariance, without a device."""
    from libviso_amd import kitti_shard
    L = kitti_shard.load_host()
    recs = _random_records(np.random.default_rng(21), 3)
    recs[0]["status"], recs[0]["cov"] = 0, 0
    recs["n"] = [0, 17, 1200]
    recs["sigma2"] = [0.0, 0.1 / 3, 2.0 / 7]
    recs["gap"] = [0.0, 1e-300, 12.5]
    f = tmp_path / "sub" / "cov.txt"
    assert L.viso_kitti_write_covariances(str(f).encode(), recs.ctypes.data, 3) == 1
    lines = f.read_text().splitlines()
    assert len(lines) == 3
    iu = np.triu_indices(6)
    for line, c in zip(lines, recs):
        v = line.split()
        assert len(v) == 25 and int(v[0]) == c["status"] and int(v[1]) == c["n"]
        assert float(v[2]) == c["sigma2"] and float(v[3]) == c["gap"]                 # %.17g round-trips
        assert [float(x) for x in v[4:]] == c["cov"][iu].tolist()
    for mode, s in ((3, 0.0), (-1, 0.0), (2, 0.0), (2, -1.0), (2, float("nan")), (2, float("inf"))):
        assert L.viso_kitti_set_covariance(mode, s) == -1
    assert L.viso_kitti_set_covariance(2, 0.5) == 1 and L.viso_kitti_set_covariance(0, 0.0) == 1
    assert L.viso_kitti_write_covariances(None, recs.ctypes.data, 3) == -1
    assert L.viso_kitti_write_covariances(str(f).encode(), None, 3) == -1
    with pytest.raises(SystemExit):   # --covariance-sigma belongs to --covariance
        kitti_shard.main(["sha", "00", "--covariance-sigma", "0.5"])
