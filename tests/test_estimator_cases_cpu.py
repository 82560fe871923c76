"""No-GPU checks of the cases and bounds the device tests of the fp64 motion estimators rest on (tests/estimator_cases.py,
tests/estimator_util.py): every far start takes the branch it is listed for and decides it robustly, `slack` is what it says,
no per-case bound is wider than the fixed one it replaced, and the seam cases are what the device tests assume."""
import numpy as np
import pytest

from libviso_amd import synth

import covariance_ref as CR
import estimator_cases as EC
import refine_ref as RR
import window_cases as WC
import window_ref as WR
from estimator_util import (PTS_REL, PTS_WHITE, TR_WHITE, WIN_ABS, ambiguous, bound, raw_bound, tr_abs_limits)

FAR = [s for s, tags in sorted(EC.CASES.items()) if "record_fails" not in tags]
RECORD_FAILS = [s for s, tags in sorted(EC.CASES.items()) if "record_fails" in tags]


def _stable(figures, what):
    for k, (diff, limit) in figures.items():
        assert diff <= 0.1 * limit, (what, k, diff, limit)


@pytest.mark.parametrize("s", FAR)
def test_far_start_takes_its_branch_and_decides_it_robustly(s):
    with np.errstate(all="ignore"):
        want = RR.refine(*EC.refine_case(s), 1)
    assert want["status"] == 1
    assert EC.tags_of(want) == EC.CASES[s], (s, EC.tags_of(want), want["trace"])
    if "max_accept" in EC.CASES[s] or "max_reject" in EC.CASES[s]:
        assert not ambiguous(want), (s, want["trace"])         # so the device's iters must be equal
        assert want["gap"] > 1e-6, (s, want["gap"])            # and the run did not converge
    assert len(EC.decisions(want["trace"])) >= len(want["trace"]) - 2, (s, want["trace"])
    for k in range(EC.N_ORDERS):
        with np.errstate(all="ignore"):
            other = RR.refine(*EC.refine_case(s, order=k), 1)
        assert other["status"] == 1
        assert EC.decisions(want["trace"]) == EC.decisions(other["trace"]), (s, k, want["trace"], other["trace"])
        _stable(EC.refine_stability(want, other, EC.permutation(100, k)), (s, k))


def test_count_cases_pin_the_number_of_rejections(monkeypatch):
    assert set(EC.COUNT_CASES) <= {s for s, tags in EC.CASES.items() if "max_reject" in tags}
    for mod, run in ((RR, lambda s: RR.refine(*EC.refine_case(s), 1)),
                     (WR, lambda s: WR.window(EC.window_case(s)[0], 2, 3, EC.window_case(s)[1], 1))):
        for s in (EC.COUNT_CASES if mod is RR else (293,)):
            with np.errstate(all="ignore"):
                want = run(s)
                monkeypatch.setattr(mod, "MAX_REJECT", 9)
                more = run(s)
                monkeypatch.setattr(mod, "MAX_REJECT", 7)
                fewer = run(s)
                monkeypatch.setattr(mod, "MAX_REJECT", 8)
            assert more["iters"] > want["iters"] and abs(more["cost"] - want["cost"]) > 1e-3 * want["cost"], s
            # one rejection fewer cannot show: a rejected step moves nothing
            assert fewer["iters"] == want["iters"] and fewer["cost"] == want["cost"], s


@pytest.mark.parametrize("s", RECORD_FAILS)
def test_far_start_fails_at_the_record_robustly(s):
    args = EC.refine_case(s)
    want, log = EC.refine_logged(*args)
    assert want["status"] == -2 and want["tr"].tobytes() == np.asarray(args[2]).tobytes()
    logs = [log]
    for k in range(EC.N_ORDERS):
        other, log_p = EC.refine_logged(*EC.refine_case(s, order=k))
        assert other["status"] == -2 and len(log) == len(log_p), (s, k, len(log), len(log_p))
        logs.append(log_p)
    for lg in logs:
        assert len(lg) >= 10 and lg[-1][4] == 0.0 and all(e[4] > 0.0 for e in lg[:-1]), (s, len(lg))
        P, tr, z0, z1, _lam = lg[-1]
        assert not np.array_equal(tr, args[2])                 # the loop moved tr before the record failed
        assert EC.points_missing_the_pivot_test(P, tr, z0, z1, args[4]) >= 5, s


@pytest.mark.parametrize("s", sorted(EC.WINDOW_CASES))
def test_window_far_start_takes_its_branch_and_decides_it_robustly(s):
    frames, param = EC.window_case(s)
    with np.errstate(all="ignore"):
        want = WR.window(frames, 2, 3, param, 1)
    assert want["status"] == 1 and want["len"] == 3 and want["n_points"] >= 60
    assert EC.tags_of(want) == EC.WINDOW_CASES[s], (s, EC.tags_of(want), want["trace"])
    assert (want["gap"] > 1e-6) == (s == 293) and (s != 293 or not ambiguous(want)), (s, want["gap"])
    assert len(EC.decisions(want["trace"])) >= len(want["trace"]) - 2, (s, want["trace"])
    for k in range(EC.N_ORDERS):
        with np.errstate(all="ignore"):
            other = WR.window(EC.window_case(s, order=k)[0], 2, 3, param, 1)
        assert other["status"] == 1 and other["n_points"] == want["n_points"]
        assert EC.decisions(want["trace"]) == EC.decisions(other["trace"]), (s, k, want["trace"], other["trace"])
        _stable(EC.window_stability(want, other), (s, k))


def test_slack_is_the_last_accepted_and_one_further_step():
    X, obs, tr, param = synth.make_solver_case(40, m=40, outlier_frac=0.0)
    inl = np.arange(40)
    want, log = EC.refine_logged(X, obs, tr, inl, param)
    assert want["status"] == 1 and want["iters"] >= 2 and want["trace"][-1] < 0     # the last decision accepted a step
    # the systems: one per decision, then the record's (lam = 0), then the further step's
    assert len(log) == len(want["trace"]) + 2 and log[-2][4] == 0.0
    P, trv, z0, z1, lam = log[-1]
    assert np.array_equal(P, want["points"]) and np.array_equal(trv, want["tr"])
    assert lam == max(log[-3][4] / 10.0, RR.LAMBDA_MIN)                               # what the loop would use next
    Cinv = np.linalg.inv(want["cov"])
    pmax = np.abs(want["points"]).max()
    further = RR.step_sizes(RR.lm_step(P, trv, z0, z1, param, lam), Cinv, want["Hpp"], pmax)
    Pl, trl = log[-3][0], log[-3][1]                                                  # the state the last accepted step left
    last = RR.step_sizes((want["tr"] - trl, want["points"] - Pl), Cinv, want["Hpp"], pmax)
    for k, v in want["slack"].items():
        assert v > 0 and abs(v - max(last[k], further[k])) <= 1e-3 * v, (k, v, last[k], further[k])
    # the window's restatement at K = 2 is the same problem: its slack is the same
    frames, _trs, wparam = WC.simulate(np.random.default_rng(3), 3)
    for t in (1, 2):
        fr = frames[t]
        w, r = WR.window(frames, t, 2, wparam, 1), RR.refine(fr.X, fr.obs, fr.tr, fr.inl, wparam, 1)
        for k, v in r["slack"].items():
            assert abs(w["slack"][k] - v) <= 1e-3 * v, (t, k, w["slack"][k], v)
    # records that were never refined have none
    assert RR.refine(X, obs, tr, inl[:5], param, 1)["slack"] == RR.ZERO_SLACK


def _no_wider(want, limits_abs, what, points=True):
    sl = want["slack"]
    rows = (("tr whitened", TR_WHITE, sl["tr_white"]), ("tr absolute", limits_abs, sl["tr_abs"]),
            ("points relative", PTS_REL, sl["pts_rel"]), ("points whitened", PTS_WHITE, sl["pts_white"]))
    for name, limits, v in rows[:4 if points else 2]:
        assert raw_bound(limits, v) <= limits[1], (what, name, v)
        assert bound(limits, v) == raw_bound(limits, v)
    return [raw_bound(TR_WHITE, sl["tr_white"]), raw_bound(limits_abs, sl["tr_abs"])]


def test_no_refine_bound_is_wider_than_the_fixed_one_it_replaced():
    worst = np.zeros(2)
    for m in (6, 7, 40, 257, 1200):
        for noise in (0.0, 0.3, 1.0):
            X, obs, tr, param = synth.make_solver_case(m, m=m, outlier_frac=0.0)
            obs = obs + np.random.default_rng(m).normal(0, noise, obs.shape)
            want = RR.refine(X, obs, tr, np.arange(m), param, 1)
            assert want["status"] == 1 and ambiguous(want), (m, noise)      # a converged run always ends at rounding level
            worst = np.maximum(worst, _no_wider(want, tr_abs_limits(m), (m, noise)))
    for n in EC.SEAMS:
        want = RR.refine(*EC.seam_case(n, clean=True), 1)
        assert want["status"] == 1 and want["n"] == n
        # tr only: no fixed bound of the points was in use at these sizes, and a far point's depth is held loosely enough that
        # its last steps (2.8e-7 relative at n = 512) reach the cap of the points' bound, which then is the bound
        worst = np.maximum(worst, _no_wider(want, tr_abs_limits(n), n, points=False))
    # the same with its outliers
    worst = np.maximum(worst, _no_wider(RR.refine(*EC.seam_case(63), 1), tr_abs_limits(63), 63, points=False))
    want = RR.refine(*EC.dropped_case(), 1)
    worst = np.maximum(worst, _no_wider(want, tr_abs_limits(want["n"]), "dropped"))
    print(f"\nwidest refine bounds: tr whitened {worst[0]:.2e} (fixed: 1e-4), tr absolute {worst[1]:.2e} (fixed: 1e-6)")


def test_no_window_bound_is_wider_than_the_fixed_one_it_replaced():
    cases = [WC.hand_case(name) + (name,) for name in sorted(WC.HAND_CASES)]
    cases += [WC.chunk_case(length, n) + ((length, n),) for length in (2, 3, 4, 5) for n in WC.chunk_sizes(length)]
    worst = np.zeros(2)
    n_valid = 0
    for frames, param, expected, what in cases:
        with np.errstate(all="ignore"):
            want = WR.window(frames, len(frames) - 1, len(frames), param, 1)
        if want["status"] != 1:
            assert want["slack"] == RR.ZERO_SLACK
            continue
        n_valid += 1
        sl = want["slack"]
        assert raw_bound(TR_WHITE, sl["tr_white"]) <= TR_WHITE[1] and raw_bound(WIN_ABS, sl["tr_abs"]) <= WIN_ABS[1], (what, sl)
        worst = np.maximum(worst, [raw_bound(TR_WHITE, sl["tr_white"]), raw_bound(WIN_ABS, sl["tr_abs"])])
    assert n_valid >= 30
    print(f"\nwidest window bounds: tr whitened {worst[0]:.2e} (fixed: 1e-4), tr_win absolute {worst[1]:.2e} (fixed: 1e-6)")


def test_the_cap_binds_only_away_from_convergence():
    for s in FAR:
        with np.errstate(all="ignore"):
            want = RR.refine(*EC.refine_case(s), 1)
        capped = raw_bound(TR_WHITE, want["slack"]["tr_white"]) > TR_WHITE[1]
        assert capped == (want["gap"] > 1e-6), (s, want["slack"], want["gap"])


def test_seam_cases_are_what_the_device_tests_assume():
    X, obs, tr, inl, param = EC.dropped_case()
    assert sorted(inl) == list(range(300)) and not np.array_equal(inl, np.arange(300))
    Lp = RR.used_points(X, inl)
    assert len(Lp) == 296 and np.array_equal(Lp, np.delete(inl, sorted(EC.DROPPED)))
    want = RR.refine(X, obs, tr, inl, param, 1)
    assert want["status"] == 1 and want["n"] == 296 and np.array_equal(want["idx"], Lp)
    # the covariance weighs entry j of the list by the observation in column j, not inl[j]: the list's order matters
    Xc, oc, trc, perm, prm = EC.permuted_case()
    a = CR.motion_cov(Xc, oc, trc, perm, prm, 1)
    b = CR.motion_cov(Xc, oc, trc, np.sort(perm), prm, 1)
    assert a["status"] == b["status"] == 1
    assert CR.whitened_error(b["cov"], a["cov"]) > 1e-3             # the device test's tolerance is 1e-9
    for n in EC.SEAMS:
        assert CR.motion_cov(*EC.seam_case(n), 1)["status"] == 1, n


@pytest.mark.parametrize("n", EC.SEAMS)
def test_seam_cases_with_outliers_end_robustly(n):
    X, obs, tr, inl, param = EC.seam_case(n)
    order = EC.permutation(n)
    want, log = EC.refine_logged(X, obs, tr, inl, param)
    other, log_p = EC.refine_logged(X, obs, tr, order.astype(np.int32), param)
    assert want["status"] == other["status"] == (1 if n == 63 else -2) and len(log) == len(log_p) >= 10
    if n == 63:
        assert EC.decisions(want["trace"]) == EC.decisions(other["trace"])
        _stable(EC.refine_stability(want, other, order), n)
    else:
        for lg in (log, log_p):
            P, trv, z0, z1, lam = lg[-1]
            assert lam == 0.0 and EC.points_missing_the_pivot_test(P, trv, z0, z1, param) >= 3, n
