"""No-GPU checks of the opt-in sliding-window bundle adjustment (include/viso_hip.h, "window refinement"): the K = 2 identity with the
two-frame refinement, the optimum against numeric derivatives of the full cost, the Schur complement against the dense Gauss-Newton
system, hand-built links, breaks and tracks, the status cases, the expected records of the device tests' hand-built and chunk-edge
windows (tests/window_cases.py), a Monte Carlo of accuracy and consistency, argument errors, the kernel's resource usage and the
device entry points failing loudly without a device."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import MOTION_COV_DTYPE, WINDOW_RECORD_DTYPE

import covariance_ref as CR
import refine_ref as RR
import window_ref as WR
from estimator_util import kernel_resources
from window_cases import HAND_CASES, KEY_MAX, chunk_case, chunk_sizes, direct_frames, hand, hand_case, simulate, wn_chunk


def test_k2_is_the_two_frame_refinement():
    rng = np.random.default_rng(3)
    frames, _trs, param = simulate(rng, 8)
    for mode, sigma in ((1, None), (2, 0.3)):
        for t in range(1, 8):
            w = WR.window(frames, t, 2, param, mode, sigma)
            fr = frames[t]
            r = RR.refine(fr.X, fr.obs, fr.tr, fr.inl, param, mode, sigma)
            assert w["status"] == r["status"] == 1 and w["len"] == 2 and w["n_points"] == r["n"]
            assert w["n_rows"] == 7 * r["n"]
            amb = any(abs(d) < 1e-11 for d in r["trace"])
            assert abs(w["iters"] - r["iters"]) <= (1 if amb else 0)
            assert np.abs(w["tr"] - r["tr"]).max() <= (1e-6 if amb else 1e-10)
            assert np.array_equal(w["tr_win"][0], w["tr"]) and not w["tr_win"][1:].any()
            assert CR.whitened_error(r["cov"], w["cov"]) <= 1e-7
            for k in ("sigma2", "cost0", "cost"):
                assert abs(w[k] - r[k]) <= 1e-9 * r[k]


def test_converged_state_is_a_stationary_point_of_the_full_cost():
    rng = np.random.default_rng(5)
    frames, _trs, param = simulate(rng, 5, m=12)
    rec = WR.window(frames, 4, 4, param, 1)
    assert rec["status"] == 1 and rec["len"] == 4 and rec["iters"] >= 1
    W = rec["window"]
    shapes = [P.shape for P in rec["points"]]

    def unpack(x):
        trs = x[:W.nc].reshape(-1, 6)
        Ps, o = [], W.nc
        for s in shapes:
            Ps.append(x[o:o + 3 * s[1]].reshape(s[1], 3).T)
            o += 3 * s[1]
        return trs, Ps

    def grad(x):
        g = np.zeros_like(x)
        for i in range(len(x)):
            h = 1e-6 * max(1.0, abs(x[i]))
            e = np.zeros_like(x)
            e[i] = h
            g[i] = (WR.total_cost(W, *unpack(x + e)) - WR.total_cost(W, *unpack(x - e))) / (2 * h)
        return g

    x0 = np.concatenate([W.tr0.ravel()] + [P.T.ravel() for P in W.start_points()])
    x1 = np.concatenate([rec["tr_win"][:3].ravel()] + [P.T.ravel() for P in rec["points"]])
    g0, g1 = grad(x0), grad(x1)
    assert np.abs(g1).max() < 1e-5 * np.abs(g0).max(), (np.abs(g1).max(), np.abs(g0).max())
    assert rec["gap"] < 1e-6


def test_schur_block_equals_the_dense_inverse():
    rng = np.random.default_rng(9)
    frames, trs, param = simulate(rng, 5, m=10)
    for K in (2, 3, 5):
        t = 4
        a = WR.anchor(frames, t, K)
        W = WR.Window(frames, a, t, param)
        for state in (W.tr0, W.tr0 + 1e-3):
            Ps = W.start_points()
            S, s, _red, good = WR.normal_equations(W, state, Ps, 0.0)
            assert good
            H, g = WR.dense_hessian(W, state, Ps)
            Hi = np.linalg.inv(H)
            Si = np.linalg.inv(S)
            blk = Hi[W.nc - 6:W.nc, W.nc - 6:W.nc]
            assert np.abs(Si[-6:, -6:] - blk).max() <= 1e-9 * np.abs(blk).max(), K
            assert np.allclose(np.linalg.solve(S, s), (Hi @ g)[:W.nc], rtol=1e-7, atol=1e-14)


def test_links_forks_breaks_and_track_starts():
    # frame j + 1 continues frame j's keypoints through its prev-left
    f1 = [(10 + i, 0 + i) for i in range(8)]
    f2 = [(20 + i, 10 + i) for i in range(8)]
    f3 = [(30 + i, 20 + i) for i in range(8)]
    frames, param = hand([None, f1, f2, f3])
    trk = WR.tracks(frames, 0, 3)
    assert [(s, rows) for s, rows in trk] == [(0, [i, i, i]) for i in range(8)]
    # frame a's own rows are never used: anchored at 1, frame 1's rows start nothing
    trk = WR.tracks(frames, 1, 3)
    assert [(s, rows) for s, rows in trk] == [(1, [i, i]) for i in range(8)]
    # a fork on the current side (two rows of frame 3 with prev-left 20) and on the previous side (two rows of frame 1 with
    # cur-left 11): neither links; the tracks that start after the anchor take z0 from the next frame's Xp_c
    f3b = list(f3)
    f3b[1] = (31, 20)
    f1b = list(f1)
    f1b[0] = (11, 0)
    frames, param = hand([None, f1b, f2, f3b])
    trk = WR.tracks(frames, 0, 3)
    starts = {(s, rows[0]) for s, rows in trk}
    assert (0, 0) in starts and (0, 1) in starts          # frame 1 rows 0, 1 share cur-left 11
    assert (1, 1) in starts                               # so frame 2's row 1 (prev-left 11) starts its own track at s = 1
    assert (2, 0) in starts and (2, 1) in starts          # frame 3 rows 0, 1 share prev-left 20: neither links
    assert sum(len(rows) for _s, rows in trk) == 24       # every row in exactly one track
    tr1 = [rows for s, rows in trk if s == 1 and rows[0] == 1][0]
    assert tr1 == [1]
    rec = WR.window(frames, 3, 4, param, 2, 0.3)
    assert rec["status"] == 1 and rec["len"] == 4
    W = rec["window"]
    g = [g for g in W.groups if g["so"] == 2][0]
    k = list(g["ks"]).index([i for i, (s, rows) in enumerate(trk) if s == 2 and rows[0] == 0][0])
    assert np.allclose(g["z0"][:, k], RR.project0(frames[3].X[:, [0]], param)[:, 0])
    # breaks: ok = 0 at frame 2, or |L'| < 6 at frame 2, move the anchor to 2
    for oks, f2x in (([1, 1, 0, 1, 1], f2), ([1, 1, 1, 1, 1], f2[:5])):
        frames, param = hand([None, f1, f2x, f3, [(40 + i, 30 + i) for i in range(8)]], oks=oks)
        assert WR.anchor(frames, 4, 5) == 2 and WR.anchor(frames, 3, 5) == 2
        assert WR.is_break(frames[2])
        rec = WR.window(frames, 4, 5, param, 1)
        assert rec["len"] == 3
    frames, param = hand([None, f1, f2, f3, [(40 + i, 30 + i) for i in range(8)]])
    assert WR.anchor(frames, 4, 5) == 0 and WR.anchor(frames, 4, 3) == 2 and WR.anchor(frames, 1, 5) == 0


def test_status_cases():
    rng = np.random.default_rng(2)
    frames, _trs, param = simulate(rng, 4, m=20)
    assert WR.window(frames, 0, 3, param, 1)["status"] == 0
    fr = frames[3]
    frames[3] = WR.Frame(fr.X, fr.obs, fr.left, fr.tr, 0, fr.inl)
    rec = WR.window(frames, 3, 3, param, 1)
    assert rec["status"] == 0 and rec["len"] == 0 and np.array_equal(rec["tr"], fr.tr)
    frames[3] = WR.Frame(fr.X, fr.obs, fr.left, fr.tr, 1, fr.inl[:5])
    assert WR.window(frames, 3, 3, param, 1)["status"] == -1
    # one point, many times: the motions are not determined
    Xd, od = np.repeat(fr.X[:, :1], 20, axis=1), np.repeat(fr.obs[:, :1], 20, axis=1)
    frames[3] = WR.Frame(Xd, od, np.stack([np.arange(20) + 1000, np.arange(20) + 2000], 1), fr.tr, 1, np.arange(20))
    f2 = frames[2]
    frames[2] = WR.Frame(np.repeat(f2.X[:, :1], 20, axis=1), np.repeat(f2.obs[:, :1], 20, axis=1),
                         np.stack([np.arange(20) + 3000, np.arange(20) + 4000], 1), f2.tr, 1, np.arange(20))
    rec = WR.window(frames, 3, 2, param, 1)
    assert rec["status"] == -2 and rec["len"] == 2 and rec["n_points"] == 20
    assert np.array_equal(rec["tr_win"][0], fr.tr) and not rec["cov"].any() and rec["iters"] == 0
    # a point whose projection overflows: the cost is not finite
    Xh = fr.X.copy()
    Xh[2, 7] = 1e-306
    frames[3] = WR.Frame(Xh, fr.obs, fr.left, fr.tr, 1, fr.inl)
    frames[2] = f2
    assert WR.window(frames, 3, 2, param, 1)["status"] == -3   # K = 2: every row of frame 3 starts a track (its Xp_c is used)


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_cases_give_their_records(name):
    """Every hand-built window of the device tests (tests/test_gpu_window_edges.py) gives the record worked out for it by hand,
    in both modes, so that none of them passes as an easy status-1 record."""
    frames, param, (status, length, n_points) = hand_case(name)
    for mode, sigma in ((1, None), (2, 0.3)):
        with np.errstate(all="ignore"):
            rec = WR.window(frames, len(frames) - 1, len(frames), param, mode, sigma)
        assert (rec["status"], rec["len"], rec["n_points"]) == (status, length, n_points), (name, mode)
        if status == 1:
            trk = rec["window"].order
            a = len(frames) - length
            rows = sorted((s + 1 + i, r) for s, rr in trk for i, r in enumerate(rr))
            want = sorted((j, int(r)) for j in range(a + 1, len(frames)) for r in frames[j].Lp)
            assert rows == want, name                       # every entry of L'_{a+1..t} in exactly one track
            assert rec["gap"] <= 1e-6 and rec["iters"] < WR.MAX_ACCEPT, name   # converged: the device check applies unchanged


def test_hand_case_details():
    # the table is built from L' only: the second holder of key 15 (frame 1) and of key 13 (frame 2) is not in L'
    frames, _p, _w = hand_case("dropped_row")
    assert len(frames[1].Lp) == len(frames[2].Lp) == 8 and frames[1].left[8, 0] == 15 and frames[2].left[8, 1] == 13
    assert WR.tables(frames[1])[0][15] == 5 and WR.tables(frames[2])[1][13] == 3
    # a row listed twice holds its keys twice: neither links, and each entry starts a track
    frames, _p, _w = hand_case("row_twice")
    cur, prev = WR.tables(frames[2])
    assert cur[23] == -2 and prev[13] == -2
    assert [rows for s, rows in WR.tracks(frames, 0, 3) if s == 1] == [[3], [3]]
    # a key held by two or three rows of L' is -2, whichever row wrote first
    for name, j, side, key in (("fork3_prev", 2, 1, 10), ("fork3_cur", 1, 0, 10), ("extreme_keys_forked", 2, 0, KEY_MAX),
                               ("extreme_keys_forked", 3, 1, 0)):
        frames, _p, _w = hand_case(name)
        assert WR.tables(frames[j])[side][key] == -2, name
    frames, _p, _w = hand_case("extreme_keys")
    assert WR.tables(frames[1])[0][KEY_MAX] == 0 and WR.tables(frames[2])[1][KEY_MAX] == 0
    assert WR.tables(frames[2])[0][0] == 0 and WR.tables(frames[3])[1][0] == 0
    # breaks by |L'| < 6 move the anchor; |L'| = 6 does not
    for name in ("break_lp5", "empty_m0", "empty_ninl0", "break_z", "break_nan"):
        frames, _p, _w = hand_case(name)
        assert WR.is_break(frames[2]) and WR.anchor(frames, 4, 5) == 2, name
    frames, _p, _w = hand_case("lp6_mid")
    assert len(frames[2].Lp) == 6 and not WR.is_break(frames[2]) and WR.anchor(frames, 4, 5) == 0


@pytest.mark.parametrize("length", [2, 3, 4, 5])
def test_chunk_edge_windows(length):
    assert [wn_chunk(L) for L in (2, 3, 4, 5)] == [64, 37, 21, 13]
    for n in chunk_sizes(length):
        frames, param, want = chunk_case(length, n)
        rec = WR.window(frames, length - 1, length, param, 1)
        assert (rec["status"], rec["len"], rec["n_points"]) == want, (length, n)
        assert rec["n_rows"] == n * (3 + 4 * (length - 1)) and rec["gap"] <= 1e-6


def test_monte_carlo_accuracy_and_nees():
    """Simulated K = 4 windows with fresh pixel noise per frame on persistent points: the window's tr_t against the two-frame
    refinement's (K = 2) on the same draws, and the consistency of its marginal covariance."""
    rng = np.random.default_rng(12)
    sigma = 0.3
    e2, e4, nees = [], [], []
    for _ in range(150):
        frames, trs, param = simulate(rng, 4, m=40, sigma=sigma, keep=0.85)
        r2 = WR.window(frames, 3, 2, param, 2, sigma)
        r4 = WR.window(frames, 3, 4, param, 2, sigma)
        assert r2["status"] == 1 and r4["status"] == 1 and r4["len"] == 4
        e2.append(r2["tr"] - trs[3])
        e = r4["tr"] - trs[3]
        e4.append(e)
        nees.append(e @ np.linalg.solve(r4["cov"], e))
    e2, e4 = np.array(e2), np.array(e4)

    def rms(a):
        return float(np.sqrt((a ** 2).sum(1).mean()))

    rot, tra = rms(e4[:, :3]) / rms(e2[:, :3]), rms(e4[:, 3:]) / rms(e2[:, 3:])
    mean = float(np.mean(nees))
    print(f"K=4 / K=2 RMS ratio rotation {rot:.3f} translation {tra:.3f}; K=4 mean NEES {mean:.3f}")
    assert rot < 1.0 and tra < 1.0
    assert 5.6 <= mean <= 6.4


def test_window_refines_as_covariances_packs_for_the_chain():
    rng = np.random.default_rng(6)
    recs = np.zeros(3, WINDOW_RECORD_DTYPE)
    for t in (1, 2):
        Q = rng.normal(size=(6, 6)) * 1e-3
        recs[t]["cov"] = Q @ Q.T
        recs[t]["status"], recs[t]["n_points"], recs[t]["sigma2"], recs[t]["gap"] = 1, 40 + t, 0.1 * t, 1e-9 * t
        recs[t]["tr"] = rng.uniform(-0.1, 0.1, 6)
    covs = libviso_amd.window_refines_as_covariances(recs)
    assert covs.dtype == MOTION_COV_DTYPE
    for k in ("cov", "sigma2", "gap", "status"):
        assert np.array_equal(covs[k], recs[k])
    assert np.array_equal(covs["n"], recs["n_points"]) and not covs["delta"].any()
    S, valid = libviso_amd.chain_covariances(recs["tr"], [0, 1, 1], covs)
    S_ref, valid_ref = CR.chain(recs["tr"], [0, 1, 1], covs)
    assert np.array_equal(valid, valid_ref) and np.allclose(S, S_ref, rtol=1e-12, atol=0)


def _direct_frames(rng, n=3, m=20):
    frames, _trs, param = simulate(rng, n + 1, m=m)
    return direct_frames(frames), param


def test_argument_errors_return_codes():
    L = libviso_amd.load()
    rng = np.random.default_rng(1)
    frs, param = _direct_frames(rng)
    for mode, sigma in ((0, None), (3, None), (2, None), (2, 0.0), (2, -1.0), (2, float("nan")), (2, float("inf"))):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.window_refine(frs, param, mode=mode, sigma=sigma)
    for bad in ([], frs + frs[:2]):                                  # len 1 and len 6
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.window_refine(bad, param)
    X, obs, left, tr, inl = frs[1]
    for b in ((X, obs, left, tr, np.array([0, 1, X.shape[1]])), (X, obs, left, tr, np.array([-1, 2])),
              (X, obs, -left, tr, inl), (X, obs, left + (1 << 20), tr, inl)):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.window_refine([frs[0], b], param)
    for b in ((X, obs[:, :-1], left, tr, inl), (X[:2], obs, left, tr, inl), (X, obs, left[:-1], tr, inl), (X, obs, left, tr[:5], inl)):
        with pytest.raises(ValueError):
            libviso_amd.window_refine([frs[0], b], param)
    buf = np.zeros(4, WINDOW_RECORD_DTYPE)
    assert L.viso_batch_set_window_refine(None, 3, 1, 0.0) == -1
    assert L.viso_batch_set_window_refine(None, 0, 1, 0.0) == -1
    assert L.viso_batch_get_window_refine(None, 0, buf.ctypes.data) == -1
    assert L.viso_batch_get_window_refines(None, buf.ctypes.data) == -1
    rec = np.zeros((), WINDOW_RECORD_DTYPE)
    m = np.array([3, 3], np.intc)
    n = np.array([3, 3], np.intc)
    Xc = np.ones(18)
    lc = np.zeros(12, np.int32)
    tc = np.zeros(12)
    ic = np.array([0, 1, 2, 0, 1, 2], np.int32)
    f64, i32, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int)
    args = [3, m.ctypes.data_as(ip), Xc.ctypes.data_as(f64), np.ones(24).ctypes.data_as(f64), lc.ctypes.data_as(i32),
            tc.ctypes.data_as(f64), ic.ctypes.data_as(i32), n.ctypes.data_as(ip), C.byref(param), 1, 0.0, rec.ctypes.data]
    for i, v in ((0, 1), (0, 6), (1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (7, None), (8, None), (11, None)):
        a = list(args)
        a[i] = v
        assert L.viso_window_refine(*a) == -1, i


def test_kernel_has_no_scratch():
    """The kernels' resource usage is a property of the compiler's output: compile window.hip for gfx950 and read it.  Scratch is not
    allowed; the occupancy is reported."""
    res = kernel_resources("window.hip", ("window_links_kernel", "window_refine_kernel"))
    for name, (occ, scratch) in res.items():
        print(f"{name}: occupancy {occ}, scratch {scratch}")
        assert scratch == 0 and occ >= 1


def test_version_names_the_feature():
    v = libviso_amd.load().viso_version()
    assert b"0.4" in v and b"refinement" in v and b"window refinement" in v


def test_device_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rng = np.random.default_rng(4)
    frs, param = _direct_frames(rng)
    with pytest.raises(libviso_amd.VisoError, match="-2"):
        libviso_amd.window_refine(frs, param, mode=1)
