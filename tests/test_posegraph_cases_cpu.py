"""No-GPU checks behind tests/test_gpu_posegraph_edges.py: the numpy restatement of the pose graph's SE(3) math (tests/posegraph_ref.py)
against 60 digits (tests/posegraph_mp.py) on every single-edge case, and, on the restatement alone, that every case of
tests/posegraph_cases.py has the structure its comment claims: the orders of the dense factor, the edge counts, the runs and their
anchors, the long edges' fixed ends, both branches of the coefficients, the rejected first trial and the weak prior."""
import numpy as np
import pytest

import posegraph_cases as K
import posegraph_mp as MP
import posegraph_ref as R


def _rel(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


_errors = {}


def _math_errors():
    """Per case: the restatement's error of r, J_i, J_j (edge), r, J_j (prior) and Exp(xi) against 60 digits, once."""
    if not _errors:
        for c in K.math_cases():
            P = np.array([c["Pi"], c["Pj"]])
            r, Ji, Jj = R.edge_terms(P, 0, 1, c["Z"])
            mr, mJi, mJj = MP.edge_terms(c["Pi"], c["Pj"], c["Z"])
            pr, none, pJj = R.edge_terms(P, -1, 1, c["Zp"])
            mpr, mnone, mpJj = MP.edge_terms(None, c["Pj"], c["Zp"])
            assert none is None and mnone is None
            _errors[c["name"]] = dict(r=_rel(r, mr), Ji=_rel(Ji, mJi), Jj=_rel(Jj, mJj), prior_r=_rel(pr, mpr), prior_Jj=_rel(pJj, mpJj),
                                      exp=_rel(R.exp_se3(c["xi"]), MP.exp_se3(c["xi"])), residual=mr, prior_residual=mpr)
    return _errors


def test_the_restatement_holds_against_60_digits():
    """r, J_i, J_j and Exp of the restatement on every case, absolute error over the largest entry, within the case's bound
    (MATH_BOUND, and MATH_BOUND_FAR for poses 500 m out).  The same figures bound what the device may differ by, so a bound is
    set by float64 and these formulas alone: posegraph_cases.py says how."""
    for c in K.math_cases():
        e = _math_errors()[c["name"]]
        print(f"{c['name']:18s} r {e['r']:.1e}  J_i {e['Ji']:.1e}  J_j {e['Jj']:.1e}  prior r {e['prior_r']:.1e}  prior J_j {e['prior_Jj']:.1e}  "
              f"Exp {e['exp']:.1e}  (bound {c['bound']:.1e})")
    assert len(_math_errors()) == 2 * len(K.MATH_THETAS)
    for c in K.math_cases():
        e = _math_errors()[c["name"]]
        assert c["bound"] == (K.MATH_BOUND_FAR if c["far"] else K.MATH_BOUND)
        assert max(e["r"], e["Ji"], e["Jj"], e["prior_r"], e["prior_Jj"]) <= c["bound"], c["name"]
        assert e["exp"] <= K.MATH_BOUND, c["name"]


def test_every_residual_has_the_rotation_and_the_components_its_case_claims():
    for c in K.math_cases():
        e = _math_errors()[c["name"]]
        for r in (e["residual"], e["prior_residual"]):
            assert abs(np.linalg.norm(r[:3]) - c["theta"]) <= 1e-12 * max(c["theta"], 1e-3), c["name"]
            assert (np.abs(r[3:]) >= K.MIN_COMPONENT).all(), c["name"]
            if c["theta"] >= 0.0999:
                assert (np.abs(r[:3]) >= K.MIN_COMPONENT).all(), c["name"]
            else:
                assert c["theta"] < K.MIN_COMPONENT * np.sqrt(3.0) and (np.abs(r[:3]) >= 0.5 * c["theta"]).all(), c["name"]
            assert (r[:3] @ r[:3] < R.SERIES_THETA2) == (c["theta"] < 0.1), c["name"]      # which branch of the coefficients
        assert (np.linalg.norm(c["Pi"][:3, 3]) > 490.0) == c["far"] and (np.linalg.norm(c["Pj"][:3, 3]) > 490.0) == c["far"]
    thetas = sorted({c["theta"] for c in K.math_cases()})
    assert thetas == sorted(K.MATH_THETAS) and max(thetas) == 3.0
    assert sum(c["theta"] ** 2 < R.SERIES_THETA2 for c in K.math_cases()) == 8


def test_the_closed_form_exp_at_60_digits_is_the_matrix_exponential():
    """posegraph_mp's Exp is the header's closed form; mpmath's expm of the twist knows no closed form.  They agree far below
    float64, so the 60-digit side is not the header's formulas checking themselves."""
    for c in K.math_cases():
        d_exp, d_log = MP.self_check(c["xi"])
        assert d_exp < 1e-45 and d_log < 1e-45, (c["name"], d_exp, d_log)


def test_probe_graphs_are_runs_of_length_one():
    pairs = 2 * len(K.MATH_THETAS) * 7
    for shape in K.PROBE_SHAPES:
        p, fx, ij, Z, info, free, bound = K.probe_graph(shape)
        runs = K.runs_of(fx, ij)
        assert len(ij) == len(free) == pairs and len(runs) == pairs > 64
        assert all(b - a == 1 and len(anchors) == 1 for a, b, anchors in runs) and [a for a, _, _ in runs] == free.tolist()
        assert {kind for _, _, anchors in runs for kind, _ in anchors} == {"prior" if shape == "prior" else "fixed"}
        assert not any(R.is_long(int(i), int(j)) for i, j in ij)
        assert len(p) == (pairs if shape == "prior" else 2 * pairs) and fx.sum() == (0 if shape == "prior" else pairs)


@pytest.mark.parametrize("name,m,n_edges", [("n140_L16", 96, 156), ("n140_L170", 1020, 310), ("n140_L171", 1026, 311),
                                            ("n140_L177", 1062, 317), ("n140_L256", 1536, 396), ("n65_L11_strong", 66, 76)])
def test_seam_graphs_have_the_orders_their_names_claim(name, m, n_edges):
    p, fx, ij, Z, info, _ = K.graph(name)
    longs = [e for e, (i, j) in enumerate(ij) if R.is_long(int(i), int(j))]
    assert 6 * len(longs) == m == 6 * K.SEAMS[name][1] and len(ij) == n_edges
    assert (m % 32 == 0) == (name in ("n140_L16", "n140_L256"))
    assert (m > 1024) == (name in ("n140_L171", "n140_L177", "n140_L256"))
    assert (m - 32 > 1024) == (name in ("n140_L177", "n140_L256"))      # rows below the first block: a second trip
    assert (len(ij) > 256) == (name.startswith("n140") and name != "n140_L16")
    assert np.array_equal(info, info.transpose(0, 2, 1)) and fx.tolist() == [1] + [0] * (len(p) - 1)
    ratio = np.median([np.trace(info[e]) for e in longs]) / np.median([np.trace(info[e]) for e in range(len(ij)) if e not in longs])
    assert (ratio > 1e3) == (name == "n65_L11_strong")


@pytest.mark.parametrize("name", sorted(K.SHAPES))
def test_shape_graphs_have_the_structure_written_down(name):
    s = K.SHAPES[name]
    p, fx, ij, Z, info, _ = K.graph(name)
    edges = [tuple(int(x) for x in e) for e in ij]
    runs = K.runs_of(fx, ij)
    assert tuple((a, b) for a, b, _ in runs) == s["runs"] and all(anchors for _, _, anchors in runs)
    assert tuple(np.flatnonzero(fx)) == s["fixed"] and len(p) == s["n"]
    assert tuple(e for e in edges if R.is_long(*e)) == s["long"]
    for k in s["gaps"]:
        assert (k, k + 1) not in edges and (k + 1, k) not in edges
    for k in s["reverse"]:
        assert (k + 1, k) in edges and (k, k + 1) not in edges
    # the two solves of the restatement agree on it, so the dense one is a reference for the device's chain form
    F, g, H = R.linearize_dense(p, fx, ij, Z, info)
    for lam in (0.0, 1e-4):
        dense, chain = R.step_dense(H, g, fx, lam), R.step_chain(p, fx, ij, Z, info, lam)
        assert chain is not None
        if s["runs"]:
            assert np.abs(dense - chain).max() / np.abs(dense).max() <= 1e-10
        else:
            assert not dense.any() and not chain.any() and not g.any() and F > 1.0


def test_shapes_a_covers_every_listed_feature():
    p, fx, ij, Z, info, _ = K.graph("shapes_a")
    edges = [tuple(int(x) for x in e) for e in ij]
    runs = {(a, b): anchors for a, b, anchors in K.runs_of(fx, ij)}
    kinds = {ab: sorted(kind for kind, _ in anchors) for ab, anchors in runs.items()}
    n = len(p)
    assert kinds[(0, 11)] == ["prior"]                                   # a run at node 0, one prior
    assert kinds[(11, 12)] == ["prior", "prior"]                         # length one, cut by missing edges, two priors on the node
    assert kinds[(12, 20)] == ["fixed"]                                  # a chain edge to a fixed neighbour only
    assert kinds[(22, 41)] == ["fixed_reversed"]                         # a reversed chain edge to a fixed neighbour only
    assert kinds[(41, 50)] == ["fixed", "prior"] and kinds[(51, 69)] == ["fixed_reversed"]
    assert kinds[(n - 1, n)] == ["prior"]                                # length one at node n - 1
    assert fx[20] and fx[21] and (20, 21) in edges                       # adjacent fixed nodes, an edge between them
    run_of = {k: ab for ab in runs for k in range(*ab)}
    long = [e for e in edges if R.is_long(*e)]
    assert run_of[3] != run_of[30] and (3, 30) in long                   # joins two runs
    assert any(fx[i] and not fx[j] for i, j in long) and any(fx[j] and not fx[i] for i, j in long) and any(fx[i] and fx[j] for i, j in long)
    assert (8, 60) in long and (60, 8) in long                           # two on one pair, one reversed
    assert (11, 69) in long and (0, n - 1) in long and any(run_of.get(i) == run_of.get(j) and not fx[i] for i, j in long)


def test_shapes_b_ends_in_a_fixed_node_and_all_fixed_has_long_edges():
    p, fx, ij, Z, info, _ = K.graph("shapes_b")
    edges = [tuple(int(x) for x in e) for e in ij]
    assert fx[-1] and fx[5] and fx[6] and (11, 10) in edges and (3, 11) in edges and (6, 2) in edges
    runs = K.runs_of(fx, ij)
    assert sorted(kind for kind, _ in runs[0][2]) == ["prior", "prior"] and sorted(kind for kind, _ in runs[2][2]) == ["fixed", "fixed_reversed"]
    p, fx, ij, Z, info, _ = K.graph("all_fixed")
    assert fx.all() and K.runs_of(fx, ij) == [] and sum(R.is_long(int(i), int(j)) for i, j in ij) == 2


def test_the_first_trial_of_the_rejected_graph_is_rejected_on_the_restatement():
    p, fx, ij, Z, info, _ = K.rejected_graph()
    P, rep, trace = R.optimize(p, fx, ij, Z, info, max_iters=50, eps_step=1e-10)
    print("rejected graph on the restatement:", rep, "F'/F of the first trial", trace[0, 1] / trace[0, 0])
    assert rep["status"] == 1 and rep["n_rejected"] == 1 and rep["iters"] == 14 and rep["n_long"] == 4
    assert trace[0, 4] == 0.0 and trace[0, 1] / trace[0, 0] > 1.2 and trace[1:-1, 4].all() and trace[-1, 4] == 0.0
    assert trace[1, 2] == 10.0 * trace[0, 2] == 10.0 * R.LAMBDA0
    # no other decision of the run is near its threshold either (F' / F against 1 + 2^-40, max |delta| against eps_step), so the
    # device, which rounds otherwise, must make the same ones
    margin = np.abs(trace[:-1, 1] / trace[:-1, 0] - (1.0 + R.ACCEPT_SLACK))
    print("F'/F - (1 + 2^-40), nearest:", margin.min(), "; max |delta| of the last two solves:", trace[-2:, 3])
    # (the device's cost is within 1e-13 of the restatement's, test_gpu_posegraph.py's floor: a ratio moves by 2e-13 at the most)
    assert margin.min() > 5e-13 and (trace[:-1, 3] > 5e-10).all() and trace[-1, 3] < 0.9e-10
    one, rep1, _ = R.optimize(p, fx, ij, Z, info, max_iters=1, eps_step=1e-10)
    assert rep1["status"] == 2 and rep1["n_rejected"] == 1 and rep1["cost_final"] == rep1["cost_initial"] and np.array_equal(one, p)


@pytest.mark.parametrize("drift", K.ACCEPTED_DRIFTS)
def test_the_first_trial_of_the_accepted_graphs_is_accepted_with_both_branches_of_exp(drift):
    p, fx, ij, Z, info, _ = K.accepted_graph(drift)
    one, rep, trace = R.optimize(p, fx, ij, Z, info, max_iters=1, eps_step=1e-10)
    assert rep["status"] == 2 and rep["n_rejected"] == 0 and trace[0, 4] == 1.0 and trace[0, 1] < 0.8 * trace[0, 0]
    d = R.step_chain(p, fx, ij, Z, info, R.LAMBDA0)
    phi2 = (d[fx == 0, :3] ** 2).sum(axis=1)
    print(f"drift {drift}: F'/F {trace[0, 1] / trace[0, 0]:.3f}, |phi|^2 of the first step {phi2.min():.2e} .. {phi2.max():.2e}, "
          f"{(phi2 < R.SERIES_THETA2).sum()} below the switch")
    if drift == 0.05:
        assert (phi2 < 0.7 * R.SERIES_THETA2).sum() >= 2 and (phi2 > 1.4 * R.SERIES_THETA2).sum() >= 2
    else:
        assert phi2.max() > 1.5 ** 2 and phi2.max() < 3.0 ** 2 and ((phi2 > 0.2) & (phi2 < 0.9)).sum() >= 2


def test_the_weak_prior_fails_the_chain_factor_at_lambda_zero_only():
    p, fx, ij, Z, info, _ = K.weak_prior_graph()
    assert not fx.any() and [a[:2] for a in K.runs_of(fx, ij)] == [(0, 12)] and not any(R.is_long(int(i), int(j)) for i, j in ij)
    assert R.step_chain(p, fx, ij, Z, info, 0.0) is None
    for lam in (1e-4, 1.0):
        chain = R.step_chain(p, fx, ij, Z, info, lam)
        F, g, H = R.linearize_dense(p, fx, ij, Z, info)
        assert chain is not None and np.abs(chain - R.step_dense(H, g, fx, lam)).max() / np.abs(chain).max() <= 1e-9
    for weight in (1e-10, 1e-30):      # the outcome does not hang on the weight
        info2 = info.copy()
        info2[-1] = weight * np.eye(6)
        assert R.step_chain(p, fx, ij, Z, info2, 0.0) is None and R.step_chain(p, fx, ij, Z, info2, 1e-4) is not None
