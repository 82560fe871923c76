"""Cases and checks shared by the CPU and the device tests of the opt-in sliding-window bundle adjustment (include/viso_hip.h, "window
refinement"): simulated sequences, hand-built windows with forks, breaks, duplicate entries, extreme keys and empty frames, the
windows at the edges of the kernel's track chunks, and the comparison of a device record with the restatement's (tests/window_ref.py).

A case is a window [None, Frame(1), ..., Frame(len - 1)] whose every frame is solved (ok = 1), so that the direct call
(libviso_amd.window_refine, K = len) and WR.window(frames, len - 1, len, ...) describe the same record; breaks come from |L'| < 6
alone."""
import numpy as np

from libviso_amd import synth
from libviso_amd.abi import Param

import covariance_ref as CR
import window_ref as WR
from estimator_util import TR_WHITE, WIN_ABS, bound, check_gap, check_iters, note_gap

ZERO_FIELDS = ("cov", "sigma2", "cost0", "cost", "gap", "iters")
KEY_MAX = (1 << 20) - 1                 # the largest keypoint index the direct call takes (its largest table)


def kitti_param():
    return Param.default(base=synth.KITTI_BASE, f=synth.KITTI_F, cu=synth.KITTI_CU, cv=synth.KITTI_CV)


def wn_chunk(length):
    """CH: the tracks per chunk of window.hip's camera-block assembly at window length len (64, 37, 21, 13 for len 2..5)."""
    slot = (3 * (length - 1) + 4) * (6 * (length - 1)) + 30
    return min(5632 // slot, 64)


def simulate(rng, nf, m=40, sigma=0.3, keep=0.8, zmin=8.0, zmax=40.0):
    """A sequence of nf frames with persistent points (each survives a frame with probability `keep`, new ones replace the others)
    and fresh N(0, sigma^2) pixel noise on every keypoint of every frame; a keypoint's index is its point's id.  Returns
    ([None, Frame(1), ...], the true motions, param); every frame starts at its true motion with every row an inlier."""
    param = kitti_param()
    f, cu, cv = param.f, param.cu, param.cv
    trs = [np.zeros(6)] + [np.concatenate([rng.uniform(-0.01, 0.01, 3), rng.uniform(-0.03, 0.03, 2), [-rng.uniform(0.3, 0.6)]])
                           for _ in range(nf - 1)]
    X = synth._new_points(rng, m, 1241, 376, zmin, zmax, f, cu, cv).T.copy()
    ids = np.arange(m)
    nxt = m
    kp_prev = CR.predict(X, np.zeros(6), param)[0] + rng.normal(0, sigma, (4, m))
    frames = [None]
    for j in range(1, nf):
        Xc = CR.rot(trs[j]) @ X + trs[j][3:, None]
        kp = CR.predict(X, trs[j], param)[0] + rng.normal(0, sigma, (4, X.shape[1]))
        frames.append(WR.Frame(CR.triangulate(kp_prev, param), kp, np.stack([ids, ids], 1), trs[j], 1, np.arange(X.shape[1])))
        alive = rng.random(X.shape[1]) < keep
        k_new = int(X.shape[1] - alive.sum())
        Xn = synth._new_points(rng, k_new, 1241, 376, zmin, zmax, f, cu, cv).T.copy()
        X = np.concatenate([Xc[:, alive], Xn], 1)
        kp_prev = np.concatenate([kp[:, alive], CR.predict(Xn, np.zeros(6), param)[0] + rng.normal(0, sigma, (4, k_new))], 1)
        ids = np.concatenate([ids[alive], np.arange(nxt, nxt + k_new)])
        nxt += k_new
    return frames, np.array(trs), param


def hand(lefts, oks=None, inls=None, bad=None, sigma=0.3):
    """Frames whose rows have the (cur-left, prev-left) lefts[j] (an empty list: a frame with m = 0).  Row i of every frame sees
    point i of one static scene (tr = 0), so rows that link carry the same point; X is triangulated from noisy previous-frame
    keypoints and obs is noisy, N(0, sigma^2) pixels.  oks[j]: ok_j (default 1); inls[j]: frame j's inlier list (default every
    row); bad[j]: {row: "z" (Z <= 0) or "nan" (non-finite X)}, rows dropped from L' but kept in L."""
    rng = np.random.default_rng(0)
    param = kitti_param()
    m_all = max(len(lf) for lf in lefts[1:])
    P = np.stack([rng.uniform(-5, 5, m_all), rng.uniform(-2, 2, m_all), rng.uniform(8, 30, m_all)])
    frames = [None]
    for j in range(1, len(lefts)):
        m = len(lefts[j])
        pred = CR.predict(P[:, :m], np.zeros(6), param)[0]
        X = CR.triangulate(pred + rng.normal(0, sigma, (4, m)), param)
        obs = pred + rng.normal(0, sigma, (4, m))
        for r, how in ((bad or {}).get(j, {})).items():
            if how == "z":
                X[2, r] = -X[2, r]
            else:
                X[0, r] = np.nan
        ok = 1 if oks is None else oks[j]
        inl = np.arange(m) if inls is None or inls.get(j) is None else inls[j]
        frames.append(WR.Frame(X, obs, np.asarray(lefts[j], np.int64).reshape(-1, 2), np.zeros(6), ok, inl))
    return frames, param


def direct_frames(frames):
    """The tuple list libviso_amd.window_refine takes for the window's frames 1..len-1."""
    return [(fr.X, fr.obs, fr.left, fr.tr, fr.inl) for fr in frames[1:]]


# ---- the hand-built windows ---------------------------------------------------------------------------------------------------
# Chains of 8 rows: frame j's row i has cur-left 10 j + i and prev-left 10 (j - 1) + i, so row i links to row i of frame j - 1.
def chain(j, n=8):
    return [(10 * j + i, 10 * (j - 1) + i) for i in range(n)]


def _with(rows, **changes):
    out = list(rows)
    for i, v in changes.items():
        out[int(i[1:])] = v
    return out


def _status_case(kind):
    """test_status_cases' sequence (4 frames of 20 points) with frame 3, and for "repeated" frame 2, replaced."""
    frames, _trs, param = simulate(np.random.default_rng(2), 4, m=20)
    fr, f2 = frames[3], frames[2]
    if kind == "lp5_t":
        frames[3] = WR.Frame(fr.X, fr.obs, fr.left, fr.tr, 1, fr.inl[:5])
        return frames, param
    if kind == "repeated":       # one point, many times, in frames 2 and 3: the motions are not determined
        frames[3] = WR.Frame(np.repeat(fr.X[:, :1], 20, axis=1), np.repeat(fr.obs[:, :1], 20, axis=1),
                             np.stack([np.arange(20) + 1000, np.arange(20) + 2000], 1), fr.tr, 1, np.arange(20))
        frames[2] = WR.Frame(np.repeat(f2.X[:, :1], 20, axis=1), np.repeat(f2.obs[:, :1], 20, axis=1),
                             np.stack([np.arange(20) + 3000, np.arange(20) + 4000], 1), f2.tr, 1, np.arange(20))
        return frames, param
    Xh = fr.X.copy()                # "overflow": a point whose projection overflows, so the starting cost is not finite
    Xh[2, 7] = 1e-306
    frames[3] = WR.Frame(Xh, fr.obs, fr.left, fr.tr, 1, fr.inl)
    return frames, param


def _case(name):
    """(frames, param) of the hand-built window `name`."""
    f1, f2, f3, f4 = chain(1), chain(2), chain(3), chain(4)
    if name == "chain":
        return hand([None, f1, f2, f3])
    if name == "chain_len5":
        return hand([None, f1, f2, f3, f4])
    if name == "chain_anchor1":     # test_links_forks_breaks_and_track_starts' anchor 1: frames 1..3 of the chain as a len-3 window
        return hand([None, f2, f3])
    if name == "forks_cur_and_prev":   # its forks: frame 1 rows 0, 1 share cur-left 11; frame 3 rows 0, 1 share prev-left 20
        return hand([None, _with(f1, r0=(11, 0)), f2, _with(f3, r1=(31, 20))])
    if name == "break_lp5":         # its break: |L'_2| = 5
        return hand([None, f1, f2[:5], f3, f4])
    if name == "fork_both_sides":   # one link, both sides: frame 1 rows 0, 1 share cur-left 11 and frame 2 rows 1, 2 prev-left 11
        return hand([None, _with(f1, r0=(11, 0)), _with(f2, r2=(22, 11)), f3])
    if name == "fork3_prev":        # three rows of frame 2 with prev-left 10: one compare-and-swap winner, two later writers
        return hand([None, f1, _with(f2, r1=(21, 10), r2=(22, 10)), f3])
    if name == "fork3_cur":         # three rows of frame 1 with cur-left 10
        return hand([None, _with(f1, r1=(10, 1), r2=(10, 2)), f2, f3])
    if name == "dropped_row":       # a key held by a second row of L that is not in L' (Z <= 0, non-finite X): it still links
        return hand([None, f1 + [(15, 8)], f2 + [(28, 13)], f3], bad={1: {8: "z"}, 2: {8: "nan"}})
    if name == "row_twice":         # frame 2 lists row 3 twice (and row 7 not at all): two entries of L', so its keys are held twice
        return hand([None, f1, f2, f3], inls={2: np.array([0, 1, 2, 3, 4, 5, 6, 3])})
    if name == "extreme_keys":      # keys 0 and 2^20 - 1 on both sides of both links
        e1 = [(KEY_MAX, 0), (0, 1)] + f1[2:]
        e2 = [(0, KEY_MAX), (KEY_MAX, 0)] + f2[2:]
        e3 = [(30, 0), (31, KEY_MAX)] + f3[2:]
        return hand([None, e1, e2, e3])
    if name == "extreme_keys_forked":   # the same, with key 2^20 - 1 held twice in frame 2 and key 0 twice in frame 3
        e1 = [(KEY_MAX, 0), (0, 1)] + f1[2:]
        e2 = [(0, KEY_MAX), (KEY_MAX, 0), (KEY_MAX, 12)] + f2[3:]
        e3 = [(30, 0), (31, KEY_MAX), (32, 22), (33, 0)] + f3[4:]
        return hand([None, e1, e2, e3])
    if name == "empty_m0":          # frame 2 has no rows at all: a break
        return hand([None, f1, [], f3, f4])
    if name == "empty_ninl0":       # frame 2 has rows but no inliers: a break
        return hand([None, f1, f2, f3, f4], inls={2: np.zeros(0, np.int64)})
    if name == "break_z":           # |L'_2| = 5: three of its eight inliers have Z <= 0
        return hand([None, f1, f2, f3, f4], bad={2: {1: "z", 4: "z", 6: "z"}})
    if name == "break_nan":         # |L'_2| = 5: three of its eight inliers have a non-finite X
        return hand([None, f1, f2, f3, f4], bad={2: {0: "nan", 3: "nan", 7: "nan"}})
    if name == "lp6_mid":           # |L'_2| = 6: no break; frame 3's rows 6, 7 find no row of L'_2 and start their own tracks
        return hand([None, f1, f2, f3, f4], bad={2: {6: "z", 7: "nan"}})
    if name == "lp5_t":             # test_status_cases' |L'_t| = 5
        return _status_case("lp5_t")
    if name == "lp5_t_bad":         # |L'_t| = 5 of 8 inliers
        return hand([None, f1, f2, f3], bad={3: {2: "z", 5: "nan", 6: "z"}})
    if name == "lp6_t":             # |L'_t| = 6: formed
        return hand([None, f1, f2, f3], bad={3: {2: "z", 5: "nan"}})
    if name == "repeated_len2":     # status -2 (test_status_cases at K = 2)
        fr, param = _status_case("repeated")
        return [None, fr[3]], param
    if name == "repeated_len3":     # the same over frames 2 and 3, whose keys do not link
        fr, param = _status_case("repeated")
        return [None, fr[2], fr[3]], param
    if name == "overflow_len2":     # status -3 (test_status_cases at K = 2: every row of frame 3 starts a track)
        fr, param = _status_case("overflow")
        return [None, fr[3]], param
    raise KeyError(name)


# name: (status, len, n_points) of the window's last frame at K = len.  Worked out by hand from the links rule; the CPU tests
# assert that the restatement gives these, so that no case drifts into an easy status-1 record.
HAND_CASES = {
    "chain": (1, 4, 8),
    "chain_len5": (1, 5, 8),
    "chain_anchor1": (1, 3, 8),
    "forks_cur_and_prev": (1, 4, 12),       # + frame 2's rows 0, 1 (s = 1: no row of frame 1 holds 10, two hold 11) + frame 3's 0, 1
    "break_lp5": (1, 3, 8),                 # anchor 2: frame 3's rows start, frame 4's link
    "fork_both_sides": (1, 4, 11),          # + frame 2's rows 0, 1, 2
    "fork3_prev": (1, 4, 11),               # + frame 2's rows 0, 1, 2
    "fork3_cur": (1, 4, 11),                # + frame 2's rows 0, 1, 2 (nothing in frame 1 holds 11 or 12 alone)
    "dropped_row": (1, 4, 8),
    "row_twice": (1, 4, 12),                # + both entries of frame 2's row 3, + frame 3's rows 3 and 7
    "extreme_keys": (1, 4, 8),
    "extreme_keys_forked": (1, 4, 12),      # + frame 3's rows 0, 1, 2, 3
    "empty_m0": (1, 3, 8),
    "empty_ninl0": (1, 3, 8),
    "break_z": (1, 3, 8),
    "break_nan": (1, 3, 8),
    "lp6_mid": (1, 5, 10),
    "lp5_t": (-1, 0, 0),
    "lp5_t_bad": (-1, 0, 0),
    "lp6_t": (1, 4, 8),
    "repeated_len2": (-2, 2, 20),
    "repeated_len3": (-2, 3, 40),
    "overflow_len2": (-3, 2, 20),
}
# The other status -1 rule (n_rows - 3 n_points - 6 (len - 1) <= 0) has no case: once a window is formed every frame in (a, t] has
# |L'| >= 6 rows, each in one track, and each row adds 4 to that sum, so it is at least 24 (len - 1) - 6 (len - 1) > 0.


def hand_case(name):
    frames, param = _case(name)
    return frames, param, HAND_CASES[name]


# ---- the windows at the edges of the track chunks -----------------------------------------------------------------------------
# A formed window has at least |L'_t| >= 6 tracks, so the smallest is 6, not 1; CH + 1 leaves a last chunk of one track.
def chunk_sizes(length):
    ch = wn_chunk(length)
    return (6, ch - 1, ch, ch + 1, 2 * ch)


def chunk_case(length, n):
    """A window of len frames and exactly n tracks: n points seen by every frame (simulate with keep = 1)."""
    frames, _trs, param = simulate(np.random.default_rng(100 * length + n), length, m=n, keep=1.0)
    return frames, param, (1, length, n)


# ---- the device record against the restatement's -------------------------------------------------------------------------------
def check(got, want, what, far=False):
    for k in ("status", "len", "n_points", "n_rows"):
        assert int(got[k]) == want[k], (what, k, int(got[k]), want[k])
    for k in ("tr", "tr_win") + ZERO_FIELDS:
        assert np.all(np.isfinite(got[k])), (what, k)
    if want["status"] != 1:
        assert np.asarray(got["tr"]).tobytes() == np.asarray(want["tr"]).tobytes(), what
        assert np.asarray(got["tr_win"]).tobytes() == np.asarray(want["tr_win"]).tobytes(), what
        for k in ZERO_FIELDS:
            assert not np.any(got[k]), (what, k)
        return
    check_iters(got["iters"], want, what)
    # the bounds are per case: the strict one plus 4 x the restatement's own last steps (estimator_util.bound)
    d = np.asarray(got["tr"]) - want["tr"]
    white = float(np.sqrt(d @ np.linalg.solve(want["cov"], d)))
    white_max = bound(TR_WHITE, want["slack"]["tr_white"])
    note_gap("window tr whitened", white, white_max, what)
    if want["n_points"] >= 40:
        assert white <= white_max, (what, white, want["slack"]["tr_white"], d)
    dw = np.abs(np.asarray(got["tr_win"]) - want["tr_win"]).max()
    dw_max = bound(WIN_ABS, want["slack"]["tr_abs"])
    note_gap("window tr_win absolute", float(dw), dw_max, what)
    assert dw <= dw_max, (what, dw, want["slack"]["tr_abs"])
    S = np.asarray(got["cov"])
    assert np.array_equal(S, S.T), what
    assert CR.whitened_error(want["cov"], S) <= 1e-7, (what, CR.whitened_error(want["cov"], S))
    for k in ("sigma2", "cost0", "cost"):
        assert abs(float(got[k]) - want[k]) <= 1e-9 * max(want[k], 1e-300), (what, k, float(got[k]), want[k])
    check_gap(float(got["gap"]), want, what, far)


def check_k2_identity(w, r):
    """A K = 2 batch's window records w against the same run's motion refinement records r, frame by frame (the identity of the
    header); returns the number of valid frames compared."""
    good = 0
    for t in range(1, len(w)):
        assert int(w[t]["status"]) == int(r[t]["status"]), t
        if int(r[t]["status"]) != 1:
            continue
        good += 1
        assert abs(int(w[t]["iters"]) - int(r[t]["iters"])) <= 1, t
        d = w[t]["tr"] - r[t]["tr"]
        assert float(np.sqrt(d @ np.linalg.solve(r[t]["cov"], d))) <= 1e-4, t
        assert CR.whitened_error(r[t]["cov"], w[t]["cov"]) <= 1e-6, t
        for k in ("sigma2", "cost0", "cost"):
            assert abs(float(w[t][k]) - float(r[t][k])) <= 1e-8 * float(r[t][k]), (t, k)
        assert float(w[t]["gap"]) <= 1e-6 and int(w[t]["n_points"]) == int(r[t]["n"])
    return good
