"""The pose-graph optimiser on the device (libviso_amd/csrc/posegraph.hip) where tests/test_gpu_posegraph.py does not reach: the SE(3)
math edge by edge against a restatement that tests/test_posegraph_cases_cpu.py holds to 60 digits, pg_dense_kernel past 1024 and at
its cap, pg_cost_kernel's second trip, chains with gaps and fixed nodes, a graph with no free node, the rejected trial of the loop,
and the one pivot failure that can be reached.  The cases and what each is for are in tests/posegraph_cases.py.

Tolerances.  Single edges: gradient and step of every (edge, information matrix) pair relative to the pair's largest entry, and the
cost of the call, within 16 x the bound the restatement itself keeps against 60 digits (MATH_BOUND = 2^-45, MATH_BOUND_FAR = 2^-42
for poses 500 m out, the cost of a call that holds both kinds by the second).  The 16 is test_gpu_posegraph.py's margin for another
order of operations; here it also covers sincos against numpy's sin and cos.  Exp: the poses optimize(max_iters = 1) returns against
the restatement's retract with the device's own step, rotation entries within 16 x MATH_BOUND and translations within that times
the largest translation.  Solver seams and chain shapes: test_gpu_posegraph.py's scheme as it is (reference(), MARGIN, the floors).

Measured on an MI355X (the tests print every figure; worst over the pairs of a call, both lambdas):
  single edges, unit translations (16 x MATH_BOUND = 4.5e-13): gradient 3.8e-15 .. 6.1e-15; step 3.2e-14 .. 4.4e-14 with P_j free
    or a prior, and with P_i free 6.5e-13 at cond H = 2.4e4 (0.7 rad, Omega 6; its bound 5.3e-12)
  single edges, 500 m out (16 x MATH_BOUND_FAR = 3.6e-12): gradient 1.2e-13 .. 1.3e-13, step 5.4e-14 .. 2.9e-13; cost 5.6e-16 .. 9.0e-16
  Exp (4.5e-13): rotation entries 1.1e-16 and 2.2e-16, translations 8.2e-17 and 1.3e-16 of the largest
  seams and shapes, cost 0 .. 5.7e-16 and gradient 1.3e-15 .. 3.9e-15 (floor 1e-13); step, lambda 0 | 1e-4, (the restatement's spread):
    n140_L16   1.9e-11 (1.3e-12) | 3.6e-13 (3.5e-13)        n140_L170  3.4e-11 (2.8e-11) | 3.6e-12 (5.8e-12)
    n140_L171  4.5e-11 (3.8e-11) | 2.0e-12 (3.1e-12)        n140_L177  5.7e-11 (3.8e-11) | 3.0e-12 (5.2e-12)
    n140_L256  1.0e-10 (7.3e-11) | 3.6e-12 (9.2e-12)        n65_L11_strong  5.0e-08 (3.4e-08) | 1.6e-11 (2.0e-11)
    shapes_a   7.3e-12 (2.7e-12) | 1.8e-12 (6.9e-13)        shapes_b   2.6e-13 (2.3e-13) | 4.8e-13 (4.7e-13)
    (n140_L16 at lambda 0 is the nearest to its bound, 14.8 of the 16 spreads)
  no free node: cost 1.9e-16; weak prior at lambda 1e-4: step 6.4e-13 (spread 6.1e-13)
  rejected first trial: F' / F = 1.4316, 14 solves as on the restatement, optimum to 7.6e-15 (bound 1e-9)

Not here, on purpose.  Status -2 from viso_pose_graph_optimize and a failure of the dense factor cannot be reached decisively: the
loop's damping is relative to diag H and starts at 1e-4, which lifts every pivot of T to 1e-4 of its diagonal entry, eight orders
above the test; and S = I + U' W is the identity plus a positive semi-definite matrix, so its pivots never fall below one while W
is finite.  A case built to sit on either test would pass or fail with the rounding.  Residual rotations nearer pi than 3 rad are
outside the contract, and graphs of workload size are tools/posegraph_bench.py's."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import POSE_GRAPH_REPORT, VISO_ERR_ARG, ptr

import posegraph_cases as K
import posegraph_ref as R
import test_gpu_posegraph as G
from test_gpu_posegraph import FLOOR_STEP, FLOOR_SUMS, MARGIN, _optimize_raw, device_graph

pytestmark = pytest.mark.gpu


def reference(name):
    """test_gpu_posegraph.py's reference() on a graph of posegraph_cases.py: it takes its graphs from that module's cache."""
    G._graphs.setdefault((name, 0.01), K.graph(name))
    return G.reference(name)


def _linearize_raw(g, lam, with_step=True, ctx=None):
    """viso_pose_graph_linearize as it is: (result, error text, cost, grad, step); step_out NULL without with_step."""
    n = len(g.poses)
    cost, grad, step = C.c_double(-7.0), np.full((n, 6), -7.0), np.full((n, 6), -7.0)
    L = libviso_amd.load()
    r = L.viso_pose_graph_linearize(*g._graph_args(ctx), float(lam), C.byref(cost), ptr(grad, C.c_double),
                                    ptr(step, C.c_double) if with_step else None)
    return r, L.viso_last_error().decode(), cost.value, grad, step


# ---- B. the device against the math, edge by edge --------------------------------------------------------------------------------------
_probe_refs = {}


def _probe_reference(shape):
    if shape not in _probe_refs:
        p, fx, ij, Z, info, free, bound = K.probe_graph(shape)
        F, g, H = R.linearize_dense(p, fx, ij, Z, info)
        cond = np.array([np.linalg.cond(H[6 * k:6 * k + 6, 6 * k:6 * k + 6]) for k in free])
        _probe_refs[shape] = (F, g, {lam: R.step_dense(H, g, fx, lam) for lam in (0.0, 1e-4)}, cond)
    return _probe_refs[shape]


@pytest.mark.parametrize("lam", [0.0, 1e-4])
@pytest.mark.parametrize("shape", K.PROBE_SHAPES)
def test_single_edges_against_the_restatement(viso, shape, lam):
    """One call a shape: 140 pairs (10 residual rotations x 2 translation scales x 7 information matrices), each free node a run of
    its own.  With Omega = I + 99 e_m e_m' the gradient is nearly 100 r_m x row m of the Jacobian, and at lambda = 0 the step of a
    pair is -J^-1 r whatever Omega is: every entry of J_j (j_free, prior) and of J_i (i_free) carries weight somewhere."""
    p, fx, ij, Z, info, free, bound = K.probe_graph(shape)
    F, g, steps, cond = _probe_reference(shape)
    # the step's bound is 16 x the math's bound where the free node is P_j or has a prior.  J_i = -J_j Ad(M^-1) carries
    # [t]x of a translation of a few metres, H = J_i' Omega J_i has a condition number of 1e3 .. 4e4 on these pairs, and a Cholesky
    # solve in float64 is good to cond(H) x 2^-52 and no better, on the device as in numpy (whose two solves differ by up to 3e-13
    # there): the i_free step gets that where it is the larger.  J_i itself is held by the gradient, at the math's bound.
    bound_s = np.maximum(MARGIN * bound, cond * 2.0 ** -52) if shape == "i_free" else MARGIN * bound
    cost, grad, step = device_graph(p, fx, ij, Z, info).linearize(lam=lam)
    err_F = abs(cost - F) / F
    scale_g, scale_s = np.abs(g[free]).max(axis=1), np.abs(steps[lam][free]).max(axis=1)
    err_g = np.abs(grad[free] - g[free]).max(axis=1) / scale_g
    err_s = np.abs(step[free] - steps[lam][free]).max(axis=1) / scale_s
    names = [c["name"] for c in K.math_cases() for _ in range(7)]
    for far in (False, True):
        sel = bound == (K.MATH_BOUND_FAR if far else K.MATH_BOUND)
        wg, ws = np.argmax(np.where(sel, err_g, -1.0)), np.argmax(np.where(sel, err_s, -1.0))
        print(f"{shape} lambda {lam} {'500 m' if far else 'unit'}: grad {err_g[wg]:.2e} ({names[wg]}, Omega {wg % 7}), "
              f"step {err_s[ws]:.2e} ({names[ws]}, Omega {ws % 7}, cond H {cond[ws]:.1e}, its bound {bound_s[ws]:.2e}); "
              f"bound x 16 = {MARGIN * bound[wg]:.2e}")
    print(f"{shape} lambda {lam}: cost {err_F:.2e}")
    assert sel.sum() == 70 and scale_g.min() > 1e-3 and scale_s.min() > 1e-3
    assert (err_g <= MARGIN * bound).all(), [names[c] for c in np.flatnonzero(err_g > MARGIN * bound)]
    assert (err_s <= bound_s).all(), [names[c] for c in np.flatnonzero(err_s > bound_s)]
    assert err_F <= MARGIN * K.MATH_BOUND_FAR
    rest = np.setdiff1d(np.arange(len(p)), free)
    assert not grad[rest].any() and not step[rest].any()
    if lam == 0.0:      # the step of a pair does not depend on its information matrix: seven solves of one -J^-1 r
        s7 = step[free].reshape(-1, 7, 6)
        assert (np.abs(s7 - s7[:, :1]).max(axis=(1, 2)) <= 2.0 * bound_s.reshape(-1, 7).max(axis=1) * np.abs(s7).max(axis=(1, 2))).all()


@pytest.mark.parametrize("drift", K.ACCEPTED_DRIFTS)
def test_exp_of_the_first_accepted_step(viso, drift):
    """pg_update_kernel alone: the step of linearize(lambda = 1e-4) is, by the determinism clause, byte for byte the first step of
    optimize, whose trial is accepted on these graphs; so optimize(max_iters = 1) returns P Exp(delta) for a delta the test holds."""
    p, fx, ij, Z, info, _ = K.accepted_graph(drift)
    g = device_graph(p, fx, ij, Z, info)
    _, _, delta = g.linearize(lam=R.LAMBDA0)
    poses, rep = g.optimize(max_iters=1, eps_step=1e-10)
    assert rep["status"] == 2 and rep["iters"] == 1 and rep["n_rejected"] == 0 and rep["cost_final"] < 0.8 * rep["cost_initial"]
    assert rep["last_step"] == np.abs(delta).max()
    phi2 = (delta[fx == 0, :3] ** 2).sum(axis=1)
    if drift == 0.05:      # both branches of pg_coef
        assert (phi2 < R.SERIES_THETA2).sum() >= 2 and (phi2 >= R.SERIES_THETA2).sum() >= 2
    else:
        assert phi2.max() > 1.5 ** 2 and ((phi2 > 0.2) & (phi2 < 0.9)).sum() >= 2
    want = R.retract(p, fx, delta)
    err_R = np.abs(poses[:, :3, :3] - want[:, :3, :3]).max()
    err_t = np.abs(poses[:, :3, 3] - want[:, :3, 3]).max() / np.abs(want[:, :3, 3]).max()
    print(f"drift {drift}: |phi|^2 {phi2.min():.2e} .. {phi2.max():.2e}; rotation entries {err_R:.2e}, translations {err_t:.2e} of the largest")
    assert err_R <= MARGIN * K.MATH_BOUND and err_t <= MARGIN * K.MATH_BOUND
    assert poses[0].tobytes() == p[0].tobytes() and fx[0] == 1
    assert np.array_equal(poses[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (len(poses), 1)))


# ---- C. solver seams and chain shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 1e-4])
@pytest.mark.parametrize("name", sorted(K.SEAMS) + ["shapes_a", "shapes_b"])
def test_linearize_at_the_seams_against_the_restatement(viso, name, lam):
    p0, fx, ij, Z, info, _ = K.graph(name)
    ref = reference(name)
    n_long = sum(R.is_long(int(a), int(b)) for a, b in ij)
    if name in K.SEAMS:
        assert n_long == K.SEAMS[name][1] and (len(ij) > 256) == (n_long >= 170)
    else:
        assert n_long == len(K.SHAPES[name]["long"])
    cost, grad, step = device_graph(p0, fx, ij, Z, info).linearize(lam=lam)
    dense, chain = ref["steps"][lam]
    spread_step = np.abs(dense - chain).max() / np.abs(dense).max()
    err_F = abs(cost - ref["F"]) / abs(ref["F"])
    err_g = np.abs(grad - ref["g"]).max() / np.abs(ref["g"]).max()
    err_s = np.abs(step - dense).max() / np.abs(dense).max()
    print(f"{name} lambda {lam}: cost {err_F:.2e} (spread {ref['spread_F']:.2e}), grad {err_g:.2e} (spread {ref['spread_g']:.2e}), "
          f"step {err_s:.2e} (spread {spread_step:.2e})")
    assert err_F <= max(MARGIN * ref["spread_F"], FLOOR_SUMS)
    assert err_g <= max(MARGIN * ref["spread_g"], FLOOR_SUMS)
    assert err_s <= max(MARGIN * spread_step, FLOOR_STEP)
    assert not grad[fx != 0].any() and not step[fx != 0].any()
    assert np.abs(step[fx == 0]).max(axis=1).min() > 0.0


def test_the_cap_of_256_long_edges_twice_and_without_a_step(viso):
    """Order 1536: two calls give the same bytes, and step_out NULL gives the same cost and gradient and leaves the solve out."""
    g = device_graph(*K.graph("n140_L256")[:5])
    a, b = _linearize_raw(g, 1e-4), _linearize_raw(g, 1e-4)
    assert a[0] == 1 and b[0] == 1, a[1]
    assert a[2] == b[2] and a[3].tobytes() == b[3].tobytes() and a[4].tobytes() == b[4].tobytes() and a[4][1:].all()
    c = _linearize_raw(g, 1e-4, with_step=False)
    assert c[0] == 1 and c[2] == a[2] and c[3].tobytes() == a[3].tobytes() and (c[4] == -7.0).all()


def test_a_graph_with_no_free_node(viso):
    """n_runs == 0 with two long edges: no chain kernel is launched, S is the identity; gradient and step are zeros, the cost is the
    restatement's; optimize converges on its first solve and returns the input."""
    p0, fx, ij, Z, info, _ = K.graph("all_fixed")
    g = device_graph(p0, fx, ij, Z, info)
    F = R.cost(p0, ij, Z, info)
    for lam in (0.0, 1e-4):
        r, msg, cost, grad, step = _linearize_raw(g, lam)
        assert r == 1, msg
        print(f"all_fixed lambda {lam}: cost {abs(cost - F) / F:.2e}")
        assert abs(cost - F) / F <= FLOOR_SUMS and not grad.any() and not step.any()
    out, rep, tr = _optimize_raw(g, 50, 1e-10, 3, 3)
    rep = dict(zip(POSE_GRAPH_REPORT, rep))
    assert rep["status"] == 1 and rep["iters"] == 1 and rep["n_long"] == 2 and rep["n_rejected"] == 0 and rep["last_step"] == 0.0
    assert rep["cost_final"] == rep["cost_initial"] == cost and out.tobytes() == p0.tobytes()
    assert tr[0].tolist() == [cost, cost, R.LAMBDA0, 0.0, 0.0] and (tr[1:] == -7.0).all()


# ---- D. the rejected step ----------------------------------------------------------------------------------------------------------
_rejected = {}


def _rejected_optimum():
    if not _rejected:
        _rejected["run"] = R.optimize(*K.rejected_graph()[:5], max_iters=50, eps_step=1e-10)
    return _rejected["run"]


def test_a_rejected_first_trial_is_solved_again_at_ten_times_lambda(viso):
    p0, fx, ij, Z, info, _ = K.rejected_graph()
    want, wrep, wtrace = _rejected_optimum()
    assert wrep["status"] == 1 and wrep["n_rejected"] == 1 and wtrace[0, 4] == 0.0
    poses, rep, trace = device_graph(p0, fx, ij, Z, info).optimize(max_iters=50, eps_step=1e-10, trace=True)
    err = np.abs(poses - want).max()
    print(f"rejected: {rep}; F'/F of the first trial {trace[0, 1] / trace[0, 0]:.4f}; worst pose entry against the restatement's optimum {err:.2e}")
    assert rep["status"] == 1 and rep["iters"] == wrep["iters"] == len(trace) and rep["n_rejected"] == 1
    assert trace[:, 4].tolist() == wtrace[:, 4].tolist()
    assert trace[0, 2] == R.LAMBDA0 and trace[1, 2] == 10.0 * trace[0, 2] and trace[1, 0] == trace[0, 0]
    assert trace[0, 1] > 1.2 * trace[0, 0] and trace[1, 1] < trace[1, 0]
    assert trace[:, 2].tolist() == wtrace[:, 2].tolist()      # the same products of the same doubles
    assert err <= 1e-9
    assert poses[0].tobytes() == p0[0].tobytes()


def test_a_rejected_trial_is_never_returned(viso):
    """max_iters = 1 on the same graph: the one solve is rejected, so status 2 comes with the poses as given, never the trial."""
    p0, fx, ij, Z, info, _ = K.rejected_graph()
    out, rep, tr = _optimize_raw(device_graph(p0, fx, ij, Z, info), 1, 1e-10, 2, 2)
    rep = dict(zip(POSE_GRAPH_REPORT, rep))
    assert rep["status"] == 2 and rep["iters"] == 1 and rep["n_rejected"] == 1 and rep["cost_final"] == rep["cost_initial"]
    assert rep["lambda"] == 10.0 * R.LAMBDA0 and tr[0, 4] == 0.0 and tr[0, 1] > 1.2 * tr[0, 0] and (tr[1] == -7.0).all()
    assert out[:, :3].tobytes() == p0[:, :3].tobytes()
    assert np.array_equal(out[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (len(out), 1)))


# ---- E. the pivot failure that can be reached --------------------------------------------------------------------------------------
def test_a_chain_that_is_not_definite_is_refused_and_the_context_goes_on(viso):
    """A prior of weight 1e-20 is an anchor to the host's check and nothing to the factor: at lambda = 0 the chain factor's last pivot
    fails its test by ten orders, the call is VISO_ERR_ARG and names the chain factor; with damping it is an ordinary solve.  A
    healthy graph on the same context gives the same bytes before and after."""
    p0, fx, ij, Z, info, _ = K.weak_prior_graph()
    weak = device_graph(p0, fx, ij, Z, info)
    healthy = device_graph(*K.graph("shapes_b")[:5])
    ctx = libviso_amd.Context(0)
    before = _linearize_raw(healthy, 0.0, ctx=ctx)
    assert before[0] == 1, before[1]
    r, msg, cost, grad, step = _linearize_raw(weak, 0.0, ctx=ctx)
    assert r == VISO_ERR_ARG and "chain factor" in msg and "lambda 0" in msg and "dense" not in msg, msg
    F, g, H = R.linearize_dense(p0, fx, ij, Z, info)
    assert abs(cost - F) / F <= FLOOR_SUMS                    # the cost and the gradient do not need the factor
    assert np.abs(grad - g).max() / np.abs(g).max() <= FLOOR_SUMS
    r, msg, cost, grad, step = _linearize_raw(weak, 0.0, with_step=False, ctx=ctx)
    assert r == 1, msg                                          # and without a step there is nothing to refuse
    r, msg, cost, grad, step = _linearize_raw(weak, 1e-4, ctx=ctx)
    assert r == 1, msg
    dense, chain = R.step_dense(H, g, fx, 1e-4), R.step_chain(p0, fx, ij, Z, info, 1e-4)
    spread = np.abs(dense - chain).max() / np.abs(dense).max()
    err_s = np.abs(step - dense).max() / np.abs(dense).max()
    print(f"weak prior, lambda 1e-4: step {err_s:.2e} (spread {spread:.2e})")
    assert err_s <= max(MARGIN * spread, FLOOR_STEP)
    after = _linearize_raw(healthy, 0.0, ctx=ctx)
    assert after[0] == 1 and after[2] == before[2] and after[3].tobytes() == before[3].tobytes() and after[4].tobytes() == before[4].tobytes()
    ctx.close()
