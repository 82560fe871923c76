"""Inputs on which the fp64 motion estimators (covariance.hip, refine.hip, window.hip) take the branches that converged runs from a
good start never reach, shared by tests/test_estimator_cases_cpu.py and tests/test_gpu_estimator_edges.py.

Far starts.  One scene (synth.make_solver_case(5, m=100, outlier_frac=0), every point an inlier) refined from
tr_true + N(0, 1) x scale x (1, 1, 1, 5, 5, 5), generator 1000 + s, scale (0.05, 0.1, 0.2, 0.3, 0.5)[s % 5].  The seeds s in CASES
were picked on the CPU with tests/refine_ref.py, by what `trace` shows (tags_of):
  rej_first       the first step is rejected, with a relative cost change d > 1e-3;
  rej_after_acc   a rejection with d > 1e-3 right after an accepted step with d < -1e-3;
  max_accept      the run ends at LM_MAX_ACCEPT (iters == 20);
  max_reject      eight rejections in a row, each with d > 1e-3: the LM_MAX_REJECT exit away from convergence;
  record_fails    the loop runs and ends, and the undamped system of the record then fails the pivot test (status -2): points that
                  an accepted step carried to |Z| ~ 1e11 and beyond have an Hpp whose pivots are rounding noise.  tr must come
                  back as it went in, after the loop moved it.
Seeds 0..699 were searched for every tag, and 700..3899 for the two exits.  None leaves the loop itself with -2 or -3: the damped
systems of this scene always pass, and the runs that end with -2 (about one in four) all do so at the record's undamped system,
as record_fails.

A far start makes the path sensitive, so a case is in the list only under a condition that tests/test_estimator_cases_cpu.py
asserts: the restatement run on each of N_ORDERS fixed permutations of the list (the same sums in other orders) takes the same
accept / reject decisions up to the first one with |d| < 1e-11, and ends within a tenth of every bound the device is held to;
for record_fails, all runs build the same number of systems and at least five points miss the pivot test by a factor of 100.
Most runs that end at an exit fail this, because 30 to 40 decisions away from convergence amplify rounding and the record's
system is badly conditioned there: other orders move the covariance of seeds 68, 77 and 179 by 2.9e-6, 2.6e-7 and 1.1e-6
whitened (the device is held to 1e-7), and the end of seed 279 by 1.6e-4.  Seed 79 shows why one order is not enough: one moves
it by 0.03 of its bounds, six by 0.16, and the device ends at 25 times the covariance's bound (2.5e-6).

A rejected step moves nothing, so a loop that allowed one rejection more or fewer leaves the same record unless the next step
would be accepted: the max_reject runs pin the exit's record, not LM_MAX_REJECT itself.  Seeds 3900..11899 were searched for
a stable run whose ninth step would be accepted, and only 9679 is one (COUNT_CASES: with nine rejections allowed it goes on to
iters = 20).  It is also the least stable case listed: its six orders reach 0.075 of a bound and the device 0.33 (the cost),
where the others stay below 0.011 and 0.03.

The window has the same branches: WINDOW_CASES are K = 3 windows (window_cases.simulate, generator 11, 60 points) whose last frame
starts as far off, found with tests/window_ref.py among seeds 0..399 under the same condition.  Seed 293 ends away from
convergence (gap 2.2) by eight rejections in a row, the last with d = 8.6e-4, so it carries no max_reject tag; a ninth step
would be accepted there too.

Seams.  seam_case(n) for n around 64, 256 and 512 (the waves inside block_sum and one lane stride of 256), and dropped_case():
300 points in a permuted list whose entries 63, 64, 255 and 256 are unusable (Z < 0, Z = 0, inf, NaN), which puts dropped points at
the wave seams and the pass seam of the compaction to L'."""
import functools

import numpy as np

from libviso_amd import synth

import covariance_ref as CR
import refine_ref as RR
import window_cases as WC
import window_ref as WR
from estimator_util import (PTS_REL, PTS_WHITE, TR_WHITE, WIN_ABS, bound, gap_tolerance, tr_abs_limits)

SCALES = (0.05, 0.1, 0.2, 0.3, 0.5)
CASES = {
    7: ("rej_first",), 8: ("rej_first",), 13: ("rej_first",), 17: ("rej_first",),
    58: ("rej_after_acc",), 154: ("rej_after_acc",),
    1143: ("rej_after_acc", "max_reject"), 1331: ("rej_after_acc", "max_reject"), 9679: ("rej_after_acc", "max_reject"),
    198: ("rej_first", "rej_after_acc", "max_accept"), 1859: ("rej_first", "rej_after_acc", "max_accept"),
    2204: ("rej_first", "rej_after_acc", "max_accept"), 3769: ("rej_first", "rej_after_acc", "max_accept"),
    288: ("record_fails",), 303: ("record_fails",),
}
COUNT_CASES = (9679,)          # a ninth step would be accepted: these pin LM_MAX_REJECT itself, the others the exit's record
WINDOW_CASES = {7: ("rej_first",), 209: ("rej_first", "rej_after_acc"), 293: ("rej_first", "rej_after_acc")}
SEAMS = (63, 64, 65, 255, 256, 257, 511, 512, 513)
DROPPED = {63: "z<0", 64: "z=0", 255: "inf", 256: "nan"}      # list position: what makes its point unusable
N_ORDERS = 6


@functools.lru_cache(maxsize=None)
def _base():
    return synth.make_solver_case(5, m=100, outlier_frac=0.0)


def far_offset(s):
    return np.random.default_rng(1000 + s).normal(size=6) * SCALES[s % 5] * np.array([1.0, 1.0, 1.0, 5.0, 5.0, 5.0])


def permutation(n, k=0):
    """The k-th fixed permutation of n entries, k < N_ORDERS."""
    return np.random.default_rng(7 + 100 * k).permutation(n)


def refine_case(s, order=None):
    """(X, obs, tr, inl, param) of far start s; order = k: the same list in the k-th fixed other order."""
    X, obs, tr_true, param = _base()
    inl = np.arange(100) if order is None else permutation(100, order)
    return X, obs, tr_true + far_offset(s), inl.astype(np.int32), param


@functools.lru_cache(maxsize=None)
def _window_base():
    return WC.simulate(np.random.default_rng(11), 3, m=60)


def window_case(s, order=None):
    """([None, Frame(1), Frame(2)], param): frame 2 starts at its true motion + far_offset(s); order = k: both inlier lists in
    their k-th fixed other order (the tracks, and so the sums, in another order)."""
    frames, _trs, param = _window_base()
    out = [None]
    for j in (1, 2):
        g = frames[j]
        inl = g.inl if order is None else g.inl[np.random.default_rng(7 + 100 * order + j).permutation(len(g.inl))]
        out.append(WR.Frame(g.X, g.obs, g.left, g.tr + far_offset(s) if j == 2 else g.tr, 1, inl))
    return out, param


def decisions(trace):
    """accept (True) / reject of every decision before the first one at rounding level."""
    out = []
    for d in trace:
        if abs(d) < 1e-11:
            break
        out.append(d < 0)
    return out


def tags_of(want):
    """The branch tags of a status-1 record, from its trace."""
    t = want["trace"]
    tags = []
    if t[0] > 1e-3:
        tags.append("rej_first")
    if any(a < -1e-3 and b > 1e-3 for a, b in zip(t[:-1], t[1:])):
        tags.append("rej_after_acc")
    if want["iters"] == RR.MAX_ACCEPT:
        tags.append("max_accept")
    if len(t) >= RR.MAX_REJECT and all(d > 1e-3 for d in t[-RR.MAX_REJECT:]):
        tags.append("max_reject")
    return tuple(tags)


def refine_logged(X, obs, tr, inl, param, mode=1, sigma=None):
    """RR.refine's record, and the (P, tr, z0, z1, lam) of every system it built -- a record that failed keeps no other trace."""
    log = []
    inner = RR.normal_equations

    def spy(P, trv, z0, z1, prm, lam):
        log.append((P, trv, z0, z1, lam))
        return inner(P, trv, z0, z1, prm, lam)

    RR.normal_equations = spy
    try:
        with np.errstate(all="ignore"):
            want = RR.refine(X, obs, tr, inl, param, mode, sigma)
    finally:
        RR.normal_equations = inner
    return want, log


def points_missing_the_pivot_test(P, tr, z0, z1, param, factor=100.0):
    """How many points' undamped Hpp miss RR.chol3_ok's pivot test with the threshold 1e-12 lowered by `factor`."""
    with np.errstate(all="ignore"):
        _J, Jx, P0, _r1, _r0 = RR.blocks(P, tr, z0, z1, param)
        A = np.einsum("nra,nrc->nac", Jx, Jx) + np.einsum("nra,nrc->nac", P0, P0)
        eps = 1e-12 / factor
        a00, a11, a22 = A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]
        l0 = np.sqrt(a00)
        l10, l20 = A[:, 1, 0] / l0, A[:, 2, 0] / l0
        p1 = a11 - l10 * l10
        l21 = (A[:, 2, 1] - l20 * l10) / np.sqrt(p1)
        p2 = a22 - l20 * l20 - l21 * l21
        good = (a00 > eps * a00) & (p1 > eps * a11) & (p2 > eps * a22)
    return int((~good).sum())


def refine_stability(want, other, order):
    """{quantity: (difference, bound)} between the restatement's record `want` and its record `other` on the list permuted by
    `order`, for every quantity the device is compared in (test_gpu_refine._check, estimator_util.check_points)."""
    sl = want["slack"]
    d = other["tr"] - want["tr"]
    dp = other["points"][:, np.argsort(order)] - want["points"]
    out = {
        "tr whitened": (float(np.sqrt(d @ np.linalg.solve(want["cov"], d))), bound(TR_WHITE, sl["tr_white"])),
        "tr absolute": (float(np.abs(d).max()), bound(tr_abs_limits(want["n"]), sl["tr_abs"])),
        "points relative": (float(np.abs(dp).max() / np.abs(want["points"]).max()), bound(PTS_REL, sl["pts_rel"])),
        "points whitened": (float(np.sqrt(np.einsum("an,nac,cn->n", dp, want["Hpp"], dp).max())),
                            bound(PTS_WHITE, sl["pts_white"])),
        "covariance": (float(CR.whitened_error(want["cov"], other["cov"])), 1e-7),
    }
    for k in ("sigma2", "cost0", "cost"):
        out[k] = (abs(other[k] - want[k]) / want[k], 1e-9)
    if want["gap"] > 1e-6:
        out["sqrt gap"] = (abs(np.sqrt(other["gap"]) - np.sqrt(want["gap"])), gap_tolerance(want))
    return out


def window_stability(want, other):
    """refine_stability for two window records (window_cases.check)."""
    sl = want["slack"]
    d = other["tr"] - want["tr"]
    out = {
        "tr whitened": (float(np.sqrt(d @ np.linalg.solve(want["cov"], d))), bound(TR_WHITE, sl["tr_white"])),
        "tr_win absolute": (float(np.abs(other["tr_win"] - want["tr_win"]).max()), bound(WIN_ABS, sl["tr_abs"])),
        "covariance": (float(CR.whitened_error(want["cov"], other["cov"])), 1e-7),
    }
    for k in ("sigma2", "cost0", "cost"):
        out[k] = (abs(other[k] - want[k]) / want[k], 1e-9)
    if want["gap"] > 1e-6:
        out["sqrt gap"] = (abs(np.sqrt(other["gap"]) - np.sqrt(want["gap"])), gap_tolerance(want))
    return out


def seam_case(n, clean=False):
    """(X, obs, tr, inl, param): n points, all listed in order, at the true motion.  A quarter of the points are outliers of up to
    40 pixels, unless clean: the covariance takes them as they are, the refinement ends with status 1 at n = 63 and, at every other
    n of SEAMS, with -2 at the record (as record_fails above: the outliers' points run away); clean, it converges in 5 steps."""
    X, obs, tr, param = synth.make_solver_case(n, m=n) if not clean else synth.make_solver_case(n, m=n, outlier_frac=0.0)
    return X, obs, tr, np.arange(n, dtype=np.int32), param


def permuted_case():
    """300 clean points listed in a fixed permutation, at the true motion."""
    X, obs, tr, param = synth.make_solver_case(9, m=300, outlier_frac=0.0)
    return X, obs, tr, permutation(300).astype(np.int32), param


def dropped_case():
    """permuted_case with the points at the list positions DROPPED made unusable: (X, obs, tr, inl, param)."""
    X, obs, tr, inl, param = permuted_case()
    X = X.copy()
    for pos, how in DROPPED.items():
        k = inl[pos]
        if how == "z<0":
            X[2, k] = -X[2, k]
        elif how == "z=0":
            X[2, k] = 0.0
        elif how == "inf":
            X[0, k] = np.inf
        else:
            X[1, k] = np.nan
    return X, obs, tr, inl, param
