"""No-GPU checks of the opt-in two-frame bundle adjustment (include/viso_hip.h, "motion refinement"): the definition's optimum
against numeric derivatives of the full cost, the Schur complement against the dense Gauss-Newton system, its accuracy and
statistical consistency (Monte Carlo, numpy), the status cases, argument errors, and the device entry points failing loudly
without a device."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MOTION_COV_DTYPE, MOTION_REFINE_DTYPE, Param

import covariance_ref as CR
import refine_ref as RR
from estimator_util import kernel_resources


def _scene(rng, m, zmin=5.0, zmax=50.0):
    """True previous-frame points (3, m) in view of both frames, a forward motion, and their exact observations in both frames."""
    f, cu, cv, b = synth.KITTI_F, synth.KITTI_CU, synth.KITTI_CV, synth.KITTI_BASE
    param = Param.default(base=b, f=f, cu=cu, cv=cv)
    tr = np.concatenate([rng.uniform(-0.02, 0.02, 3), rng.uniform(-0.05, 0.05, 2), -rng.uniform(0.5, 1.5, 1)])
    X = synth._new_points(rng, m, 1241, 376, zmin, zmax, f, cu, cv).T.copy()
    xp = CR.predict(X, np.zeros(6), param)[0]
    xc = CR.predict(X, tr, param)[0]
    return X, xp, xc, tr, param


def _noisy(rng, m, sigma):
    X, xp, xc, tr, param = _scene(rng, m)
    xpn = xp + rng.normal(0, sigma, xp.shape)
    xcn = xc + rng.normal(0, sigma, xc.shape)
    return CR.triangulate(xpn, param), xcn, tr, param


def test_converged_state_is_a_stationary_point_of_the_full_cost():
    rng = np.random.default_rng(4)
    for rep in range(3):
        Xt, obs, tr, param = _noisy(rng, 25, 0.3)
        inl = np.arange(Xt.shape[1])
        start = CR.wls(Xt, obs, inl, param, tr)
        rec = RR.refine(Xt, obs, start, inl, param, mode=1)
        assert rec["status"] == 1 and rec["n"] == 25 and rec["iters"] >= 2
        assert rec["cost"] < rec["cost0"]
        z0 = RR.project0(Xt, param)

        def grad(trv, P):
            x = np.concatenate([trv, P.T.ravel()])
            g = np.zeros_like(x)
            for i in range(len(x)):
                h = 1e-6 * max(1.0, abs(x[i]))
                e = np.zeros_like(x)
                e[i] = h
                cp = RR.cost((x + e)[6:].reshape(-1, 3).T, (x + e)[:6], z0, obs, param)
                cm = RR.cost((x - e)[6:].reshape(-1, 3).T, (x - e)[:6], z0, obs, param)
                g[i] = (cp - cm) / (2 * h)
            return g

        g0 = grad(start, Xt)
        g1 = grad(rec["tr"], rec["points"])
        assert np.abs(g1).max() < 1e-6 * np.abs(g0).max(), (rep, np.abs(g1).max(), np.abs(g0).max())
        assert rec["gap"] < 1e-6


def test_schur_complement_equals_the_dense_system():
    rng = np.random.default_rng(8)
    for m in (6, 7, 30):
        Xt, obs, tr, param = _noisy(rng, m, 0.3)
        z0 = RR.project0(Xt, param)
        for state in (tr, tr + 1e-3):
            S, s, _H, _c, _g, good = RR.normal_equations(Xt, state, z0, obs, param, 0.0)
            assert good
            H, g = RR.dense_hessian(Xt, state, z0, obs, param)
            Hi = np.linalg.inv(H)
            Si = np.linalg.inv(S)
            assert np.abs(Si - Hi[:6, :6]).max() <= 1e-9 * np.abs(Hi[:6, :6]).max(), m
            # the full Gauss-Newton step's motion part is the reduced system's
            assert np.allclose(np.linalg.solve(S, s), (Hi @ g)[:6], rtol=1e-7, atol=1e-14)


def test_monte_carlo_accuracy_and_nees():
    """1,000 noisy draws, noise in both frames: the bundle adjustment's motion against the fully converged weighted least squares
    of the current estimator (the best the reference's solver could report), and the consistency of its marginal covariance."""
    rng = np.random.default_rng(12)
    sigma = 0.3
    e_wls, e_ba, nees, s2 = [], [], [], []
    for _ in range(1000):
        Xt, obs, tr, param = _noisy(rng, 60, sigma)
        inl = np.arange(60)
        w = CR.wls(Xt, obs, inl, param, tr)
        rec = RR.refine(Xt, obs, w, inl, param, mode=2, sigma=sigma)
        assert rec["status"] == 1
        e = rec["tr"] - tr
        e_wls.append(w - tr)
        e_ba.append(e)
        nees.append(e @ np.linalg.solve(rec["cov"], e))
        s2.append(rec["cost"] / (4.0 * 60 - 6.0))
    e_wls, e_ba = np.array(e_wls), np.array(e_ba)

    def rms(a):
        return float(np.sqrt((a ** 2).sum(1).mean()))

    rot, tra = rms(e_ba[:, :3]) / rms(e_wls[:, :3]), rms(e_ba[:, 3:]) / rms(e_wls[:, 3:])
    mean = float(np.mean(nees))
    print(f"RMS ratio rotation {rot:.3f} translation {tra:.3f}; mean NEES {mean:.3f}; median sigma^2 {np.median(s2):.4f}")
    assert rot <= 0.6 and tra <= 0.6
    assert 5.6 <= mean <= 6.4
    assert abs(np.median(s2) - sigma ** 2) < 0.05 * sigma ** 2


def test_status_cases():
    rng = np.random.default_rng(2)
    Xt, obs, tr, param = _noisy(rng, 12, 0.3)
    inl = np.arange(12)
    assert RR.refine(Xt, obs, tr, inl, param, 1, ok=0)["status"] == 0
    assert RR.refine(Xt, obs, tr, inl[:5], param, 1)["status"] == -1
    bad = Xt.copy()
    bad[2, :6] = -bad[2, :6]          # Z <= 0
    bad[0, 6] = np.nan                # non-finite
    rec = RR.refine(bad, obs, tr, inl, param, 1)
    assert rec["status"] == -1 and rec["n"] == 5
    assert list(RR.used_points(bad, inl)) == list(range(7, 12))
    rec = RR.refine(bad, obs, tr, np.arange(5, 12)[::-1], param, 1)   # L' keeps L's order
    assert rec["status"] == -1 and rec["n"] == 5
    # one point, many times: the motion is not determined
    Xd, od = np.repeat(Xt[:, :1], 20, axis=1), np.repeat(obs[:, :1], 20, axis=1)
    rec = RR.refine(Xd, od, tr, np.arange(20), param, 1)
    assert rec["status"] == -2
    for r in (RR.refine(Xd, od, tr, np.arange(20), param, 1), RR.refine(Xt, obs, tr, inl[:5], param, 1)):
        assert np.array_equal(r["tr"], tr) and not r["cov"].any() and r["iters"] == 0 and r["sigma2"] == 0 and r["cost"] == 0
    # exact observations: C is rounding at the start, and the motion stays the true one
    X, xp, xc, tr0, param = _scene(rng, 10)
    rec = RR.refine(CR.triangulate(xp, param), xc, tr0, np.arange(10), param, 1)
    assert rec["status"] == 1 and rec["cost0"] < 1e-18 and rec["sigma2"] < 1e-20 and np.abs(rec["tr"] - tr0).max() < 1e-9


def test_refines_as_covariances_packs_for_the_chain():
    rng = np.random.default_rng(6)
    recs = np.zeros(3, MOTION_REFINE_DTYPE)
    for t in (1, 2):
        Q = rng.normal(size=(6, 6)) * 1e-3
        recs[t]["cov"] = Q @ Q.T
        recs[t]["status"], recs[t]["n"], recs[t]["sigma2"], recs[t]["gap"] = 1, 40 + t, 0.1 * t, 1e-9 * t
        recs[t]["tr"] = rng.uniform(-0.1, 0.1, 6)
    covs = libviso_amd.refines_as_covariances(recs)
    assert covs.dtype == MOTION_COV_DTYPE
    for k in ("cov", "sigma2", "gap", "status", "n"):
        assert np.array_equal(covs[k], recs[k])
    assert not covs["delta"].any()
    S, valid = libviso_amd.chain_covariances(recs["tr"], [0, 1, 1], covs)
    S_ref, valid_ref = CR.chain(recs["tr"], [0, 1, 1], covs)
    assert np.array_equal(valid, valid_ref) and np.allclose(S, S_ref, rtol=1e-12, atol=0)


def test_argument_errors_return_codes():
    L = libviso_amd.load()
    X, obs, tr, param = synth.make_solver_case(1, m=20, outlier_frac=0.0)
    inl = np.arange(20)
    for mode, sigma in ((0, None), (3, None), (-1, None), (2, None), (2, 0.0), (2, -1.0), (2, float("nan")), (2, float("inf"))):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.pose_refine(X, obs, tr, inl, param, mode=mode, sigma=sigma)
    for bad in (np.array([0, 1, 20]), np.array([-1, 2, 3]), np.arange(21) % 20):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.pose_refine(X, obs, tr, bad, param, mode=1)
    for Xb, ob in ((X, obs[:, :19]), (X.T, obs), (X, obs[:3]), (X[:2], obs)):
        with pytest.raises(ValueError):
            libviso_amd.pose_refine(Xb, ob, tr, inl[:5], param, mode=1)
    buf = np.zeros(4, MOTION_REFINE_DTYPE)
    assert L.viso_batch_set_refine(None, 1, 0.0) == -1
    assert L.viso_batch_get_refine(None, 0, buf.ctypes.data) == -1
    assert L.viso_batch_get_refines(None, buf.ctypes.data) == -1
    n = C.c_int(0)
    assert L.viso_batch_get_refined_points(None, 0, None, None, C.byref(n)) == -1
    rec = np.zeros((), MOTION_REFINE_DTYPE)
    f64, i32 = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    Xc, oc, tc = (np.ascontiguousarray(a, np.float64) for a in (X, obs, tr))
    ic = np.ascontiguousarray(inl, np.int32)
    args = [Xc.ctypes.data_as(f64), oc.ctypes.data_as(f64), 20, tc.ctypes.data_as(f64), ic.ctypes.data_as(i32), 20, C.byref(param), 1,
            0.0, rec.ctypes.data, None]
    for i, v in ((0, None), (1, None), (3, None), (4, None), (6, None), (9, None), (2, -1), (5, -1), (5, 21)):
        a = list(args)
        a[i] = v
        assert L.viso_pose_refine(*a) == -1, i


def test_kernel_keeps_occupancy_two_without_scratch():
    """The kernel's register budget is a property of the compiler's output: compile refine.hip for gfx950 and read the resource
    usage.  Occupancy 1 is the trap DESIGN 5.8 describes; scratch is not allowed."""
    occ, scratch = kernel_resources("refine.hip", ("motion_refine_kernel",))["motion_refine_kernel"]
    print(f"occupancy {occ}, scratch {scratch}")
    assert occ >= 2 and scratch == 0


def test_version_names_the_feature():
    v = libviso_amd.load().viso_version()
    assert b"0.4" in v and b"refinement" in v


def test_device_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    X, obs, tr, param = synth.make_solver_case(1, m=20, outlier_frac=0.0)
    with pytest.raises(libviso_amd.VisoError, match="-2"):
        libviso_amd.pose_refine(X, obs, tr, np.arange(20), param, mode=1)
