"""No-GPU checks of the pose-graph optimiser (include/viso_hip.h, "pose graph"): the numpy restatement (tests/posegraph_ref.py) against
central differences and against itself (dense solve and chain-plus-low-rank solve), its loop on a noiseless graph, the refusals and
the host-only entry points through the C ABI, the prototype table, the tool's file formats and the kernels' resource usage."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd import abi, fuse_map, posegraph
from libviso_amd.abi import MOTION_COV_DTYPE, TSDF_ALIGNMENT_DTYPE

import posegraph_ref as R
from estimator_util import kernel_resources

KERNELS = ("pg_linearize_kernel", "pg_assemble_kernel", "pg_cost_kernel", "pg_chain_factor_kernel", "pg_chain_solve_kernel",
           "pg_capacitance_kernel", "pg_dense_kernel", "pg_delta_kernel", "pg_stepmax_kernel", "pg_update_kernel")


def _numeric_jacobians(P, Z, h=1e-6):
    out = []
    for a in (0, 1):
        J = np.zeros((6, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Pp, Pm = P.copy(), P.copy()
            Pp[a], Pm[a] = P[a] @ R.exp_se3(d), P[a] @ R.exp_se3(-d)
            J[:, k] = (R.edge_terms(Pp, 0, 1, Z)[0] - R.edge_terms(Pm, 0, 1, Z)[0]) / (2 * h)
        out.append(J)
    return out


def test_jacobians_hold_against_central_differences():
    """The exact Jacobians against central differences of the restated Log at h = 1e-6, to 1e-6 (the bound of chain_covariances' G):
    large residuals, small ones on both sides of the series threshold, and a prior."""
    rng = np.random.default_rng(0)
    worst = 0.0
    for t in range(24):
        Pi, Pj = R.random_pose(rng), R.random_pose(rng)
        noise = (0.3, 1e-3, 0.05, 0.2)[t % 4]       # |phi| of the residual: 1e-3 and 0.05 take the series, 0.2 and 0.3 the closed forms
        Z = R.inv_se3(Pi) @ Pj @ R.exp_se3(rng.normal(0, noise, 6))
        P = np.array([Pi, Pj])
        _, Ji, Jj = R.edge_terms(P, 0, 1, Z)
        ni, nj = _numeric_jacobians(P, Z)
        worst = max(worst, np.abs(ni - Ji).max(), np.abs(nj - Jj).max())
    print("worst Jacobian entry against central differences:", worst)
    assert worst <= 1e-6
    P = np.array([R.random_pose(rng)])
    Z = P[0] @ R.exp_se3(rng.normal(0, 0.1, 6))
    r, Ji, Jj = R.edge_terms(P, -1, 0, Z)
    assert Ji is None
    J = np.zeros((6, 6))
    for k in range(6):
        d = np.zeros(6)
        d[k] = 1e-6
        J[:, k] = (R.edge_terms(np.array([P[0] @ R.exp_se3(d)]), -1, 0, Z)[0] - R.edge_terms(np.array([P[0] @ R.exp_se3(-d)]), -1, 0, Z)[0]) / 2e-6
    assert np.abs(J - Jj).max() <= 1e-6


def test_exp_and_log_are_inverses_across_the_series_threshold():
    rng = np.random.default_rng(1)
    for theta in (0.0, 1e-9, 1e-4, 0.05, 0.0999, 0.1001, 1.0, 3.0):
        xi = rng.normal(size=6)
        xi[:3] *= theta / np.linalg.norm(xi[:3])
        assert np.abs(R.log_se3(R.exp_se3(xi)) - xi).max() <= 1e-13, theta


@pytest.mark.parametrize("n,n_long", [(1, 0), (2, 0), (3, 1), (60, 6), (200, 3)])
def test_the_two_solves_of_the_restatement_agree(n, n_long):
    rng = np.random.default_rng(n)
    p0, fx, ij, Z, info, _ = R.make_graph(rng, n, n_long, noise=0.01, fixed=() if n < 3 else (0,), reversed_every=3, duplicates=2 if n > 2 else 0)
    F, g, H = R.linearize_dense(p0, fx, ij, Z, info)
    for lam in (0.0, 1e-4):
        a, b = R.step_dense(H, g, fx, lam), R.step_chain(p0, fx, ij, Z, info, lam)
        rel = np.abs(a - b).max() / np.abs(a).max()
        print(n, n_long, lam, "dense against chain-plus-low-rank:", rel)
        assert rel <= 1e-8


def test_a_noiseless_loop_returns_the_truth():
    rng = np.random.default_rng(5)
    p0, fx, ij, Z, info, truth = R.make_graph(rng, 40, 4, noise=0.0, n_priors=0, fixed=(0,))
    for chain in (False, True):
        P, rep, trace = R.optimize(p0, fx, ij, Z, info, eps_step=1e-10, chain=chain)
        assert rep["status"] == 1 and rep["n_long"] == 4 and np.abs(P - truth).max() <= 1e-9
        acc = trace[trace[:, 4] == 1.0]
        assert (acc[:, 1] <= acc[:, 0] * (1 + R.ACCEPT_SLACK)).all()


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------
def _call_linearize(L, poses, fixed, ij, Z, info, lam=0.0):
    poses, ij, Z, info = (np.ascontiguousarray(poses, np.float64), np.ascontiguousarray(ij, np.int32), np.ascontiguousarray(Z, np.float64),
                          np.ascontiguousarray(info, np.float64))
    fixed = None if fixed is None else np.ascontiguousarray(fixed, np.int32)
    n = len(poses.reshape(-1, 16))
    cost, grad, step = C.c_double(), np.zeros((max(n, 1), 6)), np.zeros((max(n, 1), 6))
    r = L.viso_pose_graph_linearize(None, n, abi.ptr(poses, C.c_double), abi.ptr(fixed, C.c_int32) if fixed is not None else None,
                                    len(ij.reshape(-1, 2)), abi.ptr(ij, C.c_int32), abi.ptr(Z, C.c_double), abi.ptr(info, C.c_double), lam,
                                    C.byref(cost), abi.ptr(grad, C.c_double), abi.ptr(step, C.c_double))
    return r, L.viso_last_error().decode()


def test_refusals_need_no_device(viso):
    I4, I6 = np.eye(4), np.eye(6)
    chain3 = dict(poses=[I4] * 3, ij=[(0, 1), (1, 2)], Z=[I4] * 2, info=[I6] * 2)
    # a run with neither a prior nor a fixed neighbour: named by its first node
    r, msg = _call_linearize(viso, chain3["poses"], None, chain3["ij"], chain3["Z"], chain3["info"])
    assert r == abi.VISO_ERR_ARG and "starts at node 0" in msg
    # node 1 fixed: the run {0} is anchored by its fixed neighbour, and so is {2}; the next refusal is the missing device, or none
    r, msg = _call_linearize(viso, chain3["poses"], [0, 1, 0], chain3["ij"], chain3["Z"], chain3["info"])
    assert r in (abi.VISO_OK, abi.VISO_ERR_HIP), msg
    # a gap in the chain: the second run has no anchor of its own, though a long edge reaches it
    r, msg = _call_linearize(viso, [I4] * 5, [1, 0, 0, 0, 0], [(0, 1), (1, 2), (3, 4), (1, 4)], [I4] * 4, [I6] * 4)
    assert r == abi.VISO_ERR_ARG and "starts at node 3" in msg
    # a free node with no edge at all
    r, msg = _call_linearize(viso, [I4] * 3, [1, 0, 0], [(0, 1)], [I4], [I6])
    assert r == abi.VISO_ERR_ARG and "node 2 is free and has no edge" in msg
    # edges out of range, i == j, an information matrix that is not positive definite, numbers that are not finite
    for ij in ((0, 3), (-2, 1), (1, 1), (0, -1)):
        r, msg = _call_linearize(viso, [I4] * 3, [1, 0, 0], [ij], [I4], [I6])
        assert r == abi.VISO_ERR_ARG and "edge 0 joins" in msg, ij
    bad = I6.copy()
    bad[5, 5] = 0.0
    r, msg = _call_linearize(viso, [I4] * 2, [1, 0], [(0, 1)], [I4], [bad])
    assert r == abi.VISO_ERR_ARG and "not positive definite" in msg
    nan = I4.copy()
    nan[0, 3] = np.nan
    assert _call_linearize(viso, [nan, I4], [1, 0], [(0, 1)], [I4], [I6])[0] == abi.VISO_ERR_ARG
    assert _call_linearize(viso, [I4, I4], [1, 0], [(0, 1)], [nan], [I6])[0] == abi.VISO_ERR_ARG
    assert _call_linearize(viso, [I4, I4], [1, 0], [(0, 1)], [I4], [I6], lam=-1.0)[0] == abi.VISO_ERR_ARG
    # the limits: VISO_ERR_UNSUPPORTED before anything is allocated
    n = 600
    ij = [(k, k + 1) for k in range(n - 1)] + [(0, 2 + k) for k in range(257)]
    r, msg = _call_linearize(viso, [I4] * n, [1] + [0] * (n - 1), ij, [I4] * len(ij), [I6] * len(ij))
    assert r == abi.VISO_ERR_UNSUPPORTED and "257 long edges" in msg
    r, msg = _call_linearize(viso, np.zeros((65537, 16)), None, [(0, 1)], [I4], [I6])
    assert r == abi.VISO_ERR_UNSUPPORTED
    n = 65536
    ij = [(k, k + 1) for k in range(n - 1)] + [(0, 2 + k) for k in range(200)]
    r, msg = _call_linearize(viso, np.tile(I4.reshape(16), (n, 1)), [1] + [0] * (n - 1), ij, np.tile(I4, (len(ij), 1, 1)), np.tile(I6, (len(ij), 1, 1)))
    assert r == abi.VISO_ERR_UNSUPPORTED and "workspace" in msg
    # optimise: its own arguments
    out, rep = np.zeros((2, 16)), np.zeros(8)
    args = (None, 2, abi.ptr(np.tile(I4.reshape(16), (2, 1)), C.c_double), None, 1, abi.ptr(np.array([[0, 1]], np.int32), C.c_int32),
            abi.ptr(I4.copy(), C.c_double), abi.ptr(I6.copy(), C.c_double))
    for max_iters, eps, cap in ((0, 1e-10, 0), (201, 1e-10, 0), (5, -1.0, 0), (5, np.nan, 0), (5, 1e-10, 3)):
        r = viso.viso_pose_graph_optimize(*args, max_iters, eps, abi.ptr(out, C.c_double), abi.ptr(rep, C.c_double), None, cap)
        assert r == abi.VISO_ERR_ARG, (max_iters, eps, cap)


def test_motion_edge_is_the_chain_covariance_of_a_one_edge_chain():
    rng = np.random.default_rng(2)
    for _ in range(5):
        tr = rng.normal(0, [0.02, 0.02, 0.02, 0.3, 0.3, 1.0])
        A = rng.normal(size=(6, 6))
        cov = A @ A.T * 1e-5
        Z, info = posegraph.motion_edge(tr, cov)
        covs = np.zeros(1, MOTION_COV_DTYPE)
        covs[0]["cov"], covs[0]["status"] = cov, 1
        S, valid = libviso_amd.chain_covariances(tr[None], [1], covs)
        assert valid.tolist() == [1, 1]
        assert np.abs(S[1] @ info - np.eye(6)).max() <= 1e-9 and np.array_equal(info, info.T)
        assert np.abs(Z @ libviso_amd.tr2mat(tr) - np.eye(4)).max() <= 1e-14
    with pytest.raises(libviso_amd.VisoError):
        posegraph.motion_edge(tr, np.zeros((6, 6)))
    # the batch's outputs: a failed frame pushes no pose, a frame without a covariance gets no edge; neither is bridged
    trs = rng.normal(0, 0.01, (5, 6))
    covs = np.zeros(5, MOTION_COV_DTYPE)
    covs["cov"], covs["status"] = cov, [1, 1, 0, 1, 1]
    edges, skipped = posegraph.motion_edges(trs, [1, 0, 1, 1, 1], covs)
    assert [(e[0], e[1]) for e in edges] == [(0, 1), (2, 3), (3, 4)] and skipped == [1, 2]


def test_alignment_prior_permutes_and_inverts():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(6, 6))
    rec = np.zeros((), TSDF_ALIGNMENT_DTYPE)
    rec["pose"], rec["cov"] = R.random_pose(rng), A @ A.T
    pose, info = posegraph.alignment_prior(rec)
    assert np.array_equal(pose, rec["pose"])
    cov = np.linalg.inv(info)
    assert np.allclose(cov[:3, :3], rec["cov"][3:, 3:]) and np.allclose(cov[3:, 3:], rec["cov"][:3, :3]) and np.allclose(cov[:3, 3:], rec["cov"][3:, :3])


def test_prototypes_are_in_the_table():
    i, vp, dbl = C.c_int, C.c_void_p, C.c_double
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    graph = [vp, i, f64p, i32p, i, i32p, f64p, f64p]
    assert abi.PROTOTYPES["pose_graph_linearize"] == (i, graph + [dbl, f64p, f64p, f64p])
    assert abi.PROTOTYPES["pose_graph_optimize"] == (i, graph + [i, dbl, f64p, f64p, f64p, i])
    assert abi.PROTOTYPES["motion_edge"] == (i, [f64p] * 4)
    assert len(abi.POSE_GRAPH_REPORT) == 8
    for name in ("PoseGraph", "motion_edges", "motion_edge", "alignment_prior"):
        assert callable(getattr(libviso_amd, name))


def test_files_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    p0, fx, ij, Z, info, _ = R.make_graph(rng, 20, 2, noise=0.01)
    info = 0.5 * (info + info.transpose(0, 2, 1))
    posegraph.write_edges(str(tmp_path / "e.txt"), ij, Z, info)
    ij2, Z2, info2 = posegraph.read_edges(str(tmp_path / "e.txt"))
    assert np.array_equal(ij2, ij) and ij2.dtype == np.int32
    assert np.array_equal(Z2[:, :3], Z[:, :3]) and np.array_equal(info2, info)
    fuse_map.write_poses(str(tmp_path / "p.txt"), p0)
    assert np.array_equal(fuse_map.read_poses(str(tmp_path / "p.txt"))[:, :3], p0[:, :3])
    (tmp_path / "bad.txt").write_text("0 1 2 3\n")
    with pytest.raises(ValueError):
        posegraph.read_edges(str(tmp_path / "bad.txt"))


def test_kernels_use_no_scratch():
    res = kernel_resources("posegraph.hip", KERNELS)
    for name in KERNELS:
        occ, scratch = res[name]
        assert scratch == 0 and occ >= 1, (name, occ, scratch)
