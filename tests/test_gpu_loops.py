"""The loop-closure detection on the device (include/viso_hip.h, "loop closure"; libviso_amd/csrc/loops.hip) against its numpy
restatement (tests/loop_ref.py), bit for bit: signatures, scores and candidates, the wide match, each at the sizes where a kernel
takes another path; determinism; the 52-frame scene of tests/loop_cases.py end to end through a Batch; and the purpose: the edges it
finds pull a drifted pose graph back.

The kernels' tiles: place_score_kernel works on SCORE_TILE x SCORE_TILE (j, i) cells, wide_scan_kernel on WIDE_TQ queries x WIDE_TT
targets, viso_place_candidates holds SCORE_BLOCK bytes of score rows at a time (more than one group of rows above n = 2048)."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import PoseGraph, loops, synth
from libviso_amd.abi import MatchParams

import loop_cases as LC
import loop_ref as LR
import posegraph_ref as R
from test_loops_cpu import SETUP, Z_TOL_NEAR, Z_TOL_OTHER

pytestmark = pytest.mark.gpu

SCORE_TILE, WIDE_TQ, WIDE_TT, SCORE_BLOCK = 64, 128, 64, 16 << 20


def _rows(rng, shape):
    return rng.integers(-1020, 1021, shape).astype(np.int16)


# ---- signatures ----------------------------------------------------------------------------------------------------------------------
SIG_N = np.array([0, 1, 63, 64, 65, 257, 200, 3], np.int32)


def _sig_rows():
    rng = np.random.default_rng(11)
    desc = _rows(rng, (len(SIG_N), 257, 121))
    desc[6, :50] = 0                       # all-zero rows: word 0
    desc[6, 50:60], desc[6, 60:70] = 1020, -1020
    desc[6, 70:200] = desc[6, 70]          # 130 copies of one row
    desc[7, :3] = np.array([1020, -1020] * 60 + [1020], np.int16)
    return desc


@pytest.mark.parametrize("seed", [1, 2**63 + 5])
@pytest.mark.parametrize("bits", [6, 10, 12])
def test_signatures_equal_the_restatement(viso, bits, seed):
    desc = _sig_rows()
    got = loops.place_signatures(desc, SIG_N, seed=seed, bits=bits)
    assert got.dtype == np.uint8 and got.shape == (len(SIG_N), 1 << bits)
    assert np.array_equal(got, LR.signatures(desc, SIG_N, seed, bits))
    assert not got[0].any() and got[6, 0] >= 50 and got[6].max() >= 130
    assert got.tobytes() == loops.place_signatures(desc, SIG_N, seed=seed, bits=bits).tobytes()


def test_a_bin_saturates_at_255(viso):
    desc = np.repeat(_rows(np.random.default_rng(12), (1, 1, 121)), 300, 1)
    got = loops.place_signatures(desc, [300], seed=1, bits=10)
    assert got.max() == 255 and got.sum() == 255 and np.array_equal(got, LR.signatures(desc, [300], 1, 10))


_seq = {}


def sequence():
    """Three ragged frames of libviso_amd.synth under cap = 257, their left rows as int16."""
    if not _seq:
        seq = synth.make_sequence(21, 3, n_kp=230, cap=257, ragged=True)
        _seq.update(seq=seq, left=np.ascontiguousarray(seq["desc"][:, 0]).astype(np.int16), n=np.ascontiguousarray(seq["n"][:, 0]))
    return _seq["seq"], _seq["left"], _seq["n"]


def _batch(ctx, seq, i16):
    b = libviso_amd.Batch(ctx, seq["kp"].shape[0], seq["kp"].shape[2])
    if i16:
        b.upload_i16(seq["kp"], np.ascontiguousarray(seq["desc"]).astype(np.int16), seq["n"])
    else:
        b.upload(seq["kp"], seq["desc"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=3, first_frame=0)
    return b


def test_batch_calls_equal_the_direct_calls_after_either_upload(viso):
    seq, left, n = sequence()
    pairs = [(0, 1), (1, 0), (2, 2), (2, 0), (0, 1)]
    want_sig = LR.signatures(left, n, 5, 10)
    want_m = LR.wide_match(left, n, pairs, 0.8)
    assert sum(len(m) for m in want_m) > 300
    direct = loops.place_signatures(left, n, seed=5, bits=10)
    assert np.array_equal(direct, want_sig)
    ctx = libviso_amd.Context(0)
    for i16 in (False, True):
        b = _batch(ctx, seq, i16)
        with pytest.raises(libviso_amd.VisoError, match="completed run"):
            loops.batch_place_signatures(b, seed=5, bits=10)
        with pytest.raises(libviso_amd.VisoError, match="completed run"):
            loops.batch_wide_match(b, pairs)
        b.run_matcher()
        assert loops.batch_place_signatures(b, seed=5, bits=10).tobytes() == direct.tobytes()
        assert np.array_equal(loops.batch_place_signatures(b, t0=1, t1=3, seed=5, bits=10), want_sig[1:3])
        for _ in range(2):                                   # two calls: the same rows
            got = loops.batch_wide_match(b, pairs, 0.8)
            assert len(got) == len(pairs) and all(np.array_equal(g, w) for g, w in zip(got, want_m))
        assert all(np.array_equal(g, w) for g, w in zip(loops.wide_match(left, n, pairs, 0.8, ctx=ctx), want_m))
        with pytest.raises(libviso_amd.VisoError, match="outside the range"):
            loops.batch_wide_match(b, [(0, 3)])
        b.close()
    ctx.close()


def test_batch_calls_keep_to_the_last_run_when_an_upload_follows_it(viso):
    """Rows, rank and COUNTS are the last run's: after an upload with larger counts (and other rows) and no run, the batch calls still
    answer for what ran -- never for the new counts, below which rank and the packed rows do not exist -- and after the next run for
    the new frames."""
    seq, left, n = sequence()
    big = synth.make_sequence(22, 3, n_kp=257, cap=257)
    assert (big["n"][:, 0] > n).all()
    pairs = [(0, 1), (2, 0), (1, 1)]
    ctx = libviso_amd.Context(0)
    b = _batch(ctx, seq, True)
    b.run_matcher()
    b.upload_i16(big["kp"], np.ascontiguousarray(big["desc"]).astype(np.int16), big["n"])
    for _ in range(2):
        assert np.array_equal(loops.batch_place_signatures(b, seed=5, bits=10), LR.signatures(left, n, 5, 10))
        assert all(np.array_equal(g, w) for g, w in zip(loops.batch_wide_match(b, pairs, 0.8), LR.wide_match(left, n, pairs, 0.8)))
    b.run_matcher()
    left2, n2 = np.ascontiguousarray(big["desc"][:, 0]).astype(np.int16), np.ascontiguousarray(big["n"][:, 0])
    assert np.array_equal(loops.batch_place_signatures(b, seed=5, bits=10), LR.signatures(left2, n2, 5, 10))
    assert all(np.array_equal(g, w) for g, w in zip(loops.batch_wide_match(b, pairs, 0.8), LR.wide_match(left2, n2, pairs, 0.8)))
    b.close()
    ctx.close()


def test_a_saturated_sad_is_still_a_key(viso):
    """Rows at the ends of int16 against each other: 121 * 65535 saturates at 2^18 - 2, one below what would make the key of index
    16383 the all-ones "none"; with one target the row is accepted and carries the saturated value."""
    desc = np.zeros((2, 1, 121), np.int16)
    desc[0], desc[1] = 32767, -32768
    got = loops.wide_match(desc, [1, 1], [(0, 1), (1, 0)], 0.8)
    assert [g.tolist() for g in got] == [[[0, 0, 262142]], [[0, 0, 262142]]] and LR.SAD_MAX == 262142
    assert all(np.array_equal(g, w) for g, w in zip(got, LR.wide_match(desc, [1, 1], [(0, 1), (1, 0)], 0.8)))


# ---- scores and candidates -------------------------------------------------------------------------------------------------------------
def _sigs(n, bits, seed):
    rng = np.random.default_rng(seed)
    sig = np.minimum(rng.poisson(0.6, (n, 1 << bits)), 255).astype(np.uint8)
    if n > 6:
        sig[5] = sig[2]                    # duplicate signatures: equal scores, the lower i first
        sig[4, :] = 255                    # one saturated frame
    return sig


CAND = [dict(min_gap=1, seq_len=1, nms=0, k=1), dict(min_gap=1, seq_len=3, nms=4, k=16), dict(min_gap=5, seq_len=16, nms=0, k=4),
        dict(min_gap=5, seq_len=1, nms=4, k=3, min_score="median"), dict(min_gap=1, seq_len=3, nms=0, k=4, min_score="all")]


@pytest.mark.parametrize("bits", [6, 12])
@pytest.mark.parametrize("n", [1, 2, SCORE_TILE - 1, SCORE_TILE, SCORE_TILE + 1, 2 * SCORE_TILE + 1])
def test_scores_and_candidates_equal_the_restatement(viso, n, bits):
    sig = _sigs(n, bits, 100 * n + bits)
    full = LR.scores(sig)
    for j0 in sorted({0, n // 2, n - 1}):
        got = loops.place_scores(sig, j0=j0)
        assert got.dtype == np.uint32 and np.array_equal(got, full[j0:])
        assert got.tobytes() == loops.place_scores(sig, j0=j0).tobytes()
    S = LR.sequence_sums(sig, 1)
    for kw in CAND + [dict(min_gap=n, seq_len=1, nms=0, k=2)]:
        kw = dict(kw)
        if kw.get("min_score") == "median":
            kw["min_score"] = int(np.median(S[np.tril_indices(n, -kw["min_gap"])])) if n > kw["min_gap"] else 0
        elif kw.get("min_score") == "all":
            kw["min_score"] = int(S.max()) * 16 + 1
        for j0 in sorted({0, n // 2, n - 1}):
            want = LR.candidates(sig, j0=j0, **kw)
            got = loops.place_candidates(sig, j0=j0, **kw)
            assert got[0].dtype == np.int32 and got[1].dtype == np.uint32
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (kw, j0)
        if kw.get("min_score", 0) > int(S.max()) * 16:
            assert (got[0] == -1).all() and not got[1].any()
    again = loops.place_candidates(sig, **CAND[1])
    assert again[0].tobytes() == loops.place_candidates(sig, **CAND[1])[0].tobytes()
    if n > 6:
        cand, score = loops.place_candidates(sig, min_gap=1, seq_len=1, nms=0, k=16)
        row = cand[8].tolist()                 # frames 0..7 are all kept
        assert row.index(2) < row.index(5) and score[8, row.index(2)] == score[8, row.index(5)] and row[0] == 4   # the duplicates: the lower i first
        assert ((cand >= 0).sum(1) == np.minimum(np.arange(n), 16)).all()                                      # fewer admissible frames than k


def test_saturated_histograms_at_the_longest_sequence(viso):
    """Every bin 255 at bits = 12 and seq_len = 16: the largest sum there is, 16 * 4096 * 255, in a uint32."""
    sig = np.full((20, 1 << 12), 255, np.uint8)
    cand, score = loops.place_candidates(sig, min_gap=1, seq_len=16, nms=0, k=2)
    want = LR.candidates(sig, min_gap=1, seq_len=16, nms=0, k=2)
    assert np.array_equal(cand, want[0]) and np.array_equal(score, want[1])
    assert score.max() == 16 * 4096 * 255 and cand[19].tolist() == [15, 16]      # the first i with all 16 terms, then the next


def test_candidates_over_more_than_one_group_of_rows(viso):
    """n = 2100 rows of 8400 bytes: 1997 rows fit SCORE_BLOCK, so the call takes two groups; the second one's first rows read the
    seq_len - 1 rows before them."""
    n = 2100
    assert SCORE_BLOCK // (4 * n) < n
    sig = _sigs(n, 6, 77)
    for j0 in (0, 1990):
        want = LR.candidates(sig, j0=j0, min_gap=50, seq_len=3, nms=4, k=4)
        got = loops.place_candidates(sig, j0=j0, min_gap=50, seq_len=3, nms=4, k=4)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- wide match -----------------------------------------------------------------------------------------------------------------------
WIDE_N = np.array([0, 1, 2, WIDE_TT - 1, WIDE_TT, WIDE_TT + 1, WIDE_TQ - 1, WIDE_TQ, WIDE_TQ + 1, 300, 1, 1], np.int32)
_wide = {}


def wide_case():
    """Frames of WIDE_N rows drawn from one pool of 300 base rows plus noise, so that most rows have a partner in every other frame;
    duplicated rows in frames 5 and 9 (exact ties as queries and as targets); frames 10 and 11 are one row of +1020 / -1020."""
    if not _wide:
        rng = np.random.default_rng(31)
        pool = _rows(rng, (300, 121))
        desc = np.zeros((len(WIDE_N), 300, 121), np.int16)
        for f, k in enumerate(WIDE_N):
            pick = rng.permutation(300)[:k]
            desc[f, :k] = np.clip(pool[pick] + rng.integers(-40, 41, (k, 121)), -1020, 1020)
        desc[5, 7], desc[9, 100], desc[9, 250] = desc[5, 3], desc[9, 20], desc[9, 20]
        desc[10, 0], desc[11, 0] = 1020, -1020
        pairs = [(q, t) for q in range(10) for t in range(10)] + [(9, 9), (3, 9), (10, 11), (11, 10)]
        _wide.update(desc=desc, pairs=pairs, want={r: LR.wide_match(desc, WIDE_N, pairs, r) for r in (1.0, 0.8)})
    return _wide["desc"], _wide["pairs"], _wide["want"]


@pytest.mark.parametrize("ratio", [1.0, 0.8])
def test_wide_match_equals_the_restatement(viso, ratio):
    desc, pairs, want = wide_case()
    got = loops.wide_match(desc, WIDE_N, pairs, ratio)
    assert len(got) == len(pairs)
    for (q, t), g, w in zip(pairs, got, want[ratio]):
        assert g.dtype == np.int32 and np.array_equal(g, w), (q, t, len(g), len(w))
        assert len(g) == 0 or (np.diff(g[:, 0]) > 0).all()
    by_pair = dict(zip(pairs, got))
    assert len(by_pair[(0, 9)]) == 0 and len(by_pair[(9, 0)]) == 0
    assert len(by_pair[(9, 1)]) == 1 and len(by_pair[(1, 9)]) == 1                      # one target: d2 is +inf, the mutual test decides
    assert by_pair[(10, 11)].tolist() == [[0, 0, 246840]] and by_pair[(11, 10)].tolist() == [[0, 0, 246840]]
    assert sum(len(g) for g in got) > 2000
    again = loops.wide_match(desc, WIDE_N, pairs, ratio)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))


@pytest.mark.parametrize("np_", [0, 1, 70])
def test_wide_match_pair_counts(viso, np_):
    desc, pairs, want = wide_case()
    got = loops.wide_match(desc, WIDE_N, pairs[30:30 + np_], 0.8)
    assert len(got) == np_ and all(np.array_equal(g, w) for g, w in zip(got, want[0.8][30:30 + np_]))


def test_ties_go_to_the_lower_index_both_ways(viso):
    """Equal targets: the lower one is t1, and d2 == d1 then fails the ratio test even at ratio 1.  Equal queries: the lowest owns the
    target."""
    desc, pairs, want = wide_case()
    m = dict(zip(pairs, loops.wide_match(desc, WIDE_N, pairs, 1.0)))
    same = m[(9, 9)]                                  # frame 9 against itself: rows 20, 100, 250 are one row
    assert len(same) == 297 and not {20, 100, 250} & set(same[:, 0].tolist()) and (same[:, 0] == same[:, 1]).all() and not same[:, 2].any()
    assert len(m[(5, 5)]) == WIDE_N[5] - 2 and not {3, 7} & set(m[(5, 5)][:, 0].tolist())
    owners = [set(m[(9, t)][:, 0].tolist()) & {20, 100, 250} for t in range(9)]
    assert {20} in owners and all(o <= {20} for o in owners)
    assert any(3 in m[(5, t)][:, 0].tolist() for t in range(10) if t != 5) and all(7 not in m[(5, t)][:, 0].tolist() for t in range(10))


# ---- end to end, and the purpose -------------------------------------------------------------------------------------------------------
_e2e = {}


def end_to_end():
    """The 52 frames through a Batch and detect_loops, once."""
    if not _e2e:
        case = LC.make_case(0, SETUP["n_kp"])
        ctx = libviso_amd.Context(0)
        b = libviso_amd.Batch(ctx, LC.N_FRAMES, SETUP["n_kp"])
        b.upload_i16(case["kp"], case["desc"], case["n"])
        b.set_params(MatchParams.stereo(case["F"]), MatchParams.temporal(), case["param"], seed=3, first_frame=0)
        b.run()
        details = {}
        kw = dict(seed=SETUP["seed"], bits=SETUP["bits"], min_gap=SETUP["min_gap"], seq_len=SETUP["seq_len"], nms=SETUP["nms"], k=SETUP["k"],
                  ratio=SETUP["ratio"], min_inliers=SETUP["min_inliers"])
        edges = loops.detect_loops(b, case["param"], details=details, **kw)
        frames = [((b.keypoints(t, 0), b.keypoints(t, 1)), b.matches(0, t)) for t in range(LC.N_FRAMES)]
        _e2e.update(case=case, edges=edges, details=details, frames=frames, ok=b.poses()[1])
        b.close()
        ctx.close()
    return _e2e


def test_end_to_end_equals_the_restatement_and_finds_every_revisit(viso):
    e = end_to_end()
    case, d = e["case"], e["details"]
    desc, n = case["desc"][:, 0], case["n"][:, 0]
    sig = LR.signatures(desc, n, SETUP["seed"], SETUP["bits"])
    cand, score = LR.candidates(sig, min_gap=SETUP["min_gap"], seq_len=SETUP["seq_len"], nms=SETUP["nms"], k=SETUP["k"])
    assert np.array_equal(d["sig"], sig) and np.array_equal(d["cand"], cand) and np.array_equal(d["score"], score)
    pairs = [(j, int(i)) for j in range(len(cand)) for i in cand[j] if i >= 0]
    assert d["pairs"] == pairs and len(pairs) > 40
    want = LR.wide_match(desc, n, pairs, SETUP["ratio"])
    assert all(np.array_equal(g, w) for g, w in zip(d["matches"], want))
    # the edges are those loop_edge makes of the restatement's matches
    k = 0
    for (j, i), rows in zip(pairs, want):
        if len(rows) < SETUP["min_inliers"]:
            continue
        X, obs, _ = loops.loop_observations(e["frames"][i][0], e["frames"][i][1], e["frames"][j][0], e["frames"][j][1], rows, case["param"])
        edge = loops.loop_edge(X, obs, case["param"], min_inliers=SETUP["min_inliers"], seed=0, frame=j)
        if edge is None:
            continue
        assert e["edges"][k][:2] == (i, j) and e["edges"][k][2].tobytes() == edge[0].tobytes() and e["edges"][k][3].tobytes() == edge[1].tobytes()
        k += 1
    assert k == len(e["edges"])
    worst = LC.check_edges(case, e["edges"], Z_TOL_NEAR, Z_TOL_OTHER)
    print(f"{len(e['edges'])} edges, worst |Z - truth| near / other {worst[0]:.4f} / {worst[1]:.4f}, least inliers {min(x[4] for x in e['edges'])}")
    assert loops.frame_nodes(e["ok"])[0] == 0


def test_the_loop_edges_pull_a_drifted_graph_back(viso):
    """52 nodes at the true poses' drifted chain: odometry edges are the true relative poses times Exp(N(0, 0.02)) per step, as
    posegraph_ref.make_graph draws its start, with information 1e4; the two jumps are bridged by weak edges (information 1e-2); node 0
    is fixed.  The device's loop edges are added with their own information."""
    e = end_to_end()
    truth = e["case"]["poses"]
    rng = np.random.default_rng(9)
    n = LC.N_FRAMES
    ij, Z, info = [], [], []
    p0 = [truth[0]]
    for k in range(1, n):
        Zk = R.inv_se3(truth[k - 1]) @ truth[k] @ R.exp_se3(rng.normal(0, 0.02, 6))
        ij.append((k - 1, k)); Z.append(Zk); info.append(np.eye(6) * (1e-2 if k in LC.JUMPS else 1e4))
        p0.append(p0[-1] @ Zk)
    for i, j, Ze, Oe, _ in e["edges"]:
        ij.append((i, j)); Z.append(Ze); info.append(0.5 * (Oe + Oe.T))
    p0, fx = np.array(p0), np.zeros(n, np.int32)
    fx[0] = 1
    g = PoseGraph(p0)
    for (i, j), Zk, Ok in zip(ij, Z, info):
        g.add_edge(i, j, Zk, Ok)
    g.fix(0)
    poses, rep = g.optimize(max_iters=50, eps_step=1e-10)
    want, wrep, _ = R.optimize(p0, fx, np.array(ij, np.int32), np.array(Z), np.array(info), max_iters=50, eps_step=1e-10)
    sl = slice(LC.REVISIT0, n)
    before = np.linalg.norm(p0[sl, :3, 3] - truth[sl, :3, 3], axis=1).mean()
    after = np.linalg.norm(poses[sl, :3, 3] - truth[sl, :3, 3], axis=1).mean()
    print(f"mean position error of frames 32..51: {before:.3f} m before, {after:.3f} m after; {rep}; against the restatement {np.abs(poses - want).max():.2e}")
    assert rep["status"] == 1 and wrep["status"] == 1
    assert after < before
    assert np.abs(poses - want).max() <= 1e-9
