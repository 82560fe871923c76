"""The pose-graph optimiser on the device (include/viso_hip.h, "pose graph"; libviso_amd/csrc/posegraph.hip) against its numpy
restatement (tests/posegraph_ref.py): one linearise and one solve on graphs at the sizes where the kernels change path, the loop on
noiseless and noisy graphs, determinism, the trace, and the purpose: poses optimised here move a TSDF map bit for bit.

Tolerances.  cost and grad: relative to the largest entry, 16 x the restatement's own spread when its edges are summed in a shuffled
order, with a floor of 1e-13.  step: 16 x the restatement's own spread between its dense and its chain-plus-low-rank solve on that
graph, with a floor of 1e-12.  The margin of 16 is there because the device eliminates in another order."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd import PoseGraph
from libviso_amd.abi import POSE_GRAPH_REPORT, ptr

import posegraph_ref as R
from test_tsdf_retract_cpu import MIN_DISP16, POSES, TRUNC, VOXEL, param, same, scene

pytestmark = pytest.mark.gpu

MARGIN = 16.0
FLOOR_SUMS = 1e-13   # measured spreads of cost and grad under a shuffled edge order: 0 .. 6e-16 relative (16 x is below the floor);
                     # device errors 0 .. 2.3e-14
FLOOR_STEP = 1e-12   # measured spreads between the restatement's two solves: 2.5e-16 (n = 1) .. 8.1e-12 (n = 130, lambda = 0);
                     # device errors 4e-16 .. 3.5e-11, each within 16 x its graph's spread or the floor


def _priors_only(rng, n):
    truth = R.loop_truth(n)
    ij = np.array([(-1, k) for k in range(n)], np.int32)
    Z = np.array([truth[k] @ R.exp_se3(rng.normal(0, 0.01, 6)) for k in range(n)])
    info = np.array([R.random_info(rng, 100.0) for _ in range(n)])
    p0 = np.array([truth[k] @ R.exp_se3(rng.normal(0, 0.05, 6)) for k in range(n)])
    return p0, np.zeros(n, np.int32), ij, Z, info, truth


# name -> (n_poses, n_long, make_graph's options): the smallest graphs at which each kernel takes another path
CASES = {
    "n1_prior_only": (1, 0, dict(fixed=())),
    "n2": (2, 0, dict(fixed=(0,), n_priors=0)),
    "n3_long_0_2": (3, 1, dict(fixed=())),
    "n65_L0": (65, 0, dict()),
    "n65_L1": (65, 1, dict()),
    "n65_L11_reversed_duplicates": (65, 11, dict(reversed_every=3, duplicates=5)),
    "n130_L1": (130, 1, dict()),
    "n130_L11_fixed_middle": (130, 11, dict(fixed=(64,))),
    "n130_L11_two_fixed": (130, 11, dict(fixed=(0, 64), n_priors=2)),
    "n130_L43": (130, 43, dict()),
    "n65_priors_only": (65, 0, None),
}
_graphs = {}


def graph(name, noise=0.01):
    if (name, noise) not in _graphs:
        n, L, opts = CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        g = _priors_only(rng, n) if opts is None else R.make_graph(rng, n, L, noise=noise, **opts)
        info = 0.5 * (g[4] + g[4].transpose(0, 2, 1))
        _graphs[(name, noise)] = g[:4] + (info,) + g[5:]
    return _graphs[(name, noise)]


def device_graph(p0, fx, ij, Z, info):
    g = PoseGraph(p0)
    for (i, j), Zk, Ok in zip(ij, Z, info):
        g.add_edge(i, j, Zk, Ok)
    for k in np.flatnonzero(fx):
        g.fix(k)
    return g


_refs = {}


def reference(name):
    """The restatement's linearise of a case, its spread under a shuffled edge order, and its two solves at both lambdas: once."""
    if name not in _refs:
        p0, fx, ij, Z, info, _ = graph(name)
        F, g, H = R.linearize_dense(p0, fx, ij, Z, info)
        order = np.random.default_rng(7).permutation(len(ij))
        F2, g2, _ = R.linearize_dense(p0, fx, ij, Z, info, order=order)
        steps = {lam: (R.step_dense(H, g, fx, lam), R.step_chain(p0, fx, ij, Z, info, lam)) for lam in (0.0, 1e-4)}
        _refs[name] = dict(F=F, g=g, spread_F=abs(F - F2) / abs(F), spread_g=np.abs(g - g2).max() / max(np.abs(g).max(), 1e-300), steps=steps)
    return _refs[name]


@pytest.mark.parametrize("lam", [0.0, 1e-4])
@pytest.mark.parametrize("name", sorted(CASES))
def test_linearize_against_the_restatement(viso, name, lam):
    p0, fx, ij, Z, info, _ = graph(name)
    ref = reference(name)
    assert sum(R.is_long(int(a), int(b)) for a, b in ij) == CASES[name][1]
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


def test_optimize_noiseless_loop_returns_the_truth(viso):
    """40 nodes, 4 long edges, exact Z, a drifted start: both sides stop within eps_step of a zero-cost optimum, so 10 x eps_step."""
    rng = np.random.default_rng(5)
    p0, fx, ij, Z, info, truth = R.make_graph(rng, 40, 4, noise=0.0, n_priors=0, fixed=(0,))
    poses, rep, trace = device_graph(p0, fx, ij, Z, info).optimize(eps_step=1e-10, trace=True)
    err = np.abs(poses - truth).max()
    print("noiseless:", rep, "worst pose entry", err)
    assert rep["status"] == 1 and rep["n_long"] == 4 and len(trace) == rep["iters"]
    assert err <= 1e-9
    assert np.array_equal(poses[0], p0[0])


_optima = {}


def optimum(name):
    if name not in _optima:
        _optima[name] = R.optimize(*graph(name)[:5], max_iters=50, eps_step=1e-10)
    return _optima[name]


def _optimize_raw(g, max_iters, eps_step, trace_rows, trace_cap):
    """viso_pose_graph_optimize as it is: poses_out, the report's eight words and a trace buffer of trace_rows rows filled with -7."""
    out, rep, tr = np.zeros((len(g.poses), 4, 4)), np.zeros(8), np.full((trace_rows, 5), -7.0)
    r = libviso_amd.load().viso_pose_graph_optimize(*g._graph_args(None), max_iters, eps_step, ptr(out, C.c_double), ptr(rep, C.c_double),
                                                    ptr(tr, C.c_double), trace_cap)
    assert r == 1, libviso_amd.load().viso_last_error()
    return out, rep, tr


@pytest.mark.parametrize("name", ["n65_L1", "n65_L11_reversed_duplicates", "n130_L1", "n130_L11_two_fixed"])
def test_optimize_noisy_against_the_restatement(viso, name):
    p0, fx, ij, Z, info, _ = graph(name)
    want, wrep, _ = optimum(name)
    assert wrep["status"] == 1
    g = device_graph(p0, fx, ij, Z, info)
    poses, rep, trace = g.optimize(max_iters=50, eps_step=1e-10, trace=True)
    err = np.abs(poses - want).max()
    err_F = abs(rep["cost_final"] - wrep["cost_final"]) / wrep["cost_final"]
    print(f"{name}: {rep}; worst pose entry against the restatement's optimum {err:.2e}, cost_final {err_F:.2e} (restatement: {wrep['iters']} solves)")
    assert rep["status"] == 1 and rep["n_long"] == CASES[name][1]
    assert err <= 1e-9
    assert err_F <= max(MARGIN * reference(name)["spread_F"], FLOOR_SUMS)
    acc = trace[trace[:, 4] == 1.0]
    assert len(acc) and (acc[:, 1] <= acc[:, 0] * (1 + 2.0 ** -40)).all() and (np.diff(acc[:, 1]) <= acc[1:, 1] * 2.0 ** -40).all()
    assert trace[-1, 4] == 0.0 and trace[-1, 3] <= 1e-10 and abs(trace[-1, 0] - rep["cost_final"]) == 0.0
    for k in np.flatnonzero(fx):
        assert poses[k].tobytes() == p0[k].tobytes()
    assert np.array_equal(poses[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (len(poses), 1)))
    # two calls: the same bytes; a trace_cap below the number of solves writes only its entries
    a = _optimize_raw(g, 50, 1e-10, 50, 50)
    b = _optimize_raw(g, 50, 1e-10, 50, 2)
    assert a[0].tobytes() == poses.tobytes() and a[1].tobytes() == b[1].tobytes() and a[0].tobytes() == b[0].tobytes()
    assert dict(zip(POSE_GRAPH_REPORT, a[1]))["iters"] == rep["iters"] > 2
    assert a[2][:rep["iters"]].tobytes() == trace.tobytes() and (a[2][rep["iters"]:] == -7.0).all()
    assert b[2][:2].tobytes() == trace[:2].tobytes() and (b[2][2:] == -7.0).all()
    # max_iters = 1: status 2, and the accepted first step is returned
    one, rep1 = g.optimize(max_iters=1, eps_step=1e-10)
    first = R.retract(p0, fx, R.step_dense(*R.linearize_dense(p0, fx, ij, Z, info)[:0:-1], fx, R.LAMBDA0))
    assert rep1["status"] == 2 and rep1["iters"] == 1 and rep1["n_rejected"] == 0 and rep1["cost_final"] < rep1["cost_initial"]
    assert np.abs(one - first).max() <= 1e-9 and np.abs(one - p0).max() > 1e-6


def test_a_cost_that_is_not_finite_is_status_minus_3_and_returns_the_input(viso):
    """A finite pose so far from its prior that the cost overflows: status -3, poses_out equals poses byte for byte, and the Python
    call raises with the report."""
    far = np.eye(4)
    far[:3, 3] = [1e200, -1e200, 3.0]
    p0 = np.array([far, np.eye(4)])
    g = PoseGraph(p0)
    g.add_prior(0, np.eye(4), np.eye(6))
    g.add_edge(0, 1, np.eye(4), np.eye(6))
    out, rep, tr = _optimize_raw(g, 5, 1e-10, 5, 5)
    rep = dict(zip(POSE_GRAPH_REPORT, rep))
    assert rep["status"] == -3 and rep["iters"] == 0 and out.tobytes() == p0.tobytes() and (tr == -7.0).all()
    with pytest.raises(libviso_amd.VisoError) as e:
        g.optimize(max_iters=5)
    assert e.value.report["status"] == -3


def test_optimized_poses_move_a_tsdf_map_bit_for_bit(viso):
    """The purpose: three 37 x 333 maps fused at drifted poses, a graph of their odometry edges and two priors optimised, the map moved
    to the result; its entries are those of a fresh map fused at the optimised poses."""
    rng = np.random.default_rng(11)
    frames = scene((37, 333), False)
    maps = [fr[0] for fr in frames]
    truth = np.array(POSES)
    drifted = np.array([T @ R.exp_se3(rng.normal(0, [0.004, 0.004, 0.004, 0.03, 0.03, 0.03])) for T in truth])
    g = PoseGraph(drifted)
    for k in range(2):
        g.add_edge(k, k + 1, R.inv_se3(truth[k]) @ truth[k + 1] @ R.exp_se3(rng.normal(0, 1e-3, 6)), R.random_info(rng, 1e4))
    for k in (0, 2):
        g.add_prior(k, truth[k] @ R.exp_se3(rng.normal(0, 1e-3, 6)), R.random_info(rng, 1e4))
    poses, rep = g.optimize()
    assert rep["status"] == 1 and np.abs(poses - truth).max() < np.abs(drifted - truth).max()
    kw = dict(voxel=VOXEL, trunc_voxels=TRUNC, min_disp16=MIN_DISP16, capacity_log2=18)
    moved, fresh = libviso_amd.TsdfMap(None, **kw), libviso_amd.TsdfMap(None, **kw)
    for m, T in zip(maps, drifted):
        moved.fuse(m, param(), pose=T)
    for m, T0, T1 in zip(maps, drifted, poses):
        r = moved.move(m, param(), T0, T1)
        assert r["n_missing"] == 0 and r["n_underflow"] == 0 and r["n_inconsistent"] == 0
    for m, T in zip(maps, poses):
        fresh.fuse(m, param(), pose=T)
    assert moved.stats() == fresh.stats() and moved.stats()["n_dropped"] == 0
    assert len(moved.entries()) > 1000 and same(moved.entries(), fresh.entries())
    moved.close(); fresh.close()
