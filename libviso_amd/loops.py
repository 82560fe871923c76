"""Loop-closure detection on the device (include/viso_hip.h, "loop closure"; csrc/loops.hip): place signatures of frames, the
all-pairs search for the earlier frames a frame looks like, the ungated mutual matcher between two frames, and the host glue that
turns a candidate pair's matches into an edge of posegraph.PoseGraph through the existing solver, covariance and motion_edge."""
import ctypes as C

import numpy as np

from . import _call, _ctx_h, _f32, _i32, load
from .abi import DESC_LEN, ptr
from .estimators import pose_covariance
from .plain import collect_matches, ransac_minimize_reproj, triangulate_rectified
from .posegraph import motion_edge


def _rows16(where, desc, n):
    """Descriptors [nf][cap][121] as contiguous int16 (integer values only) and their counts [nf]."""
    d = np.asarray(desc)
    if d.ndim != 3 or d.shape[2] != DESC_LEN:
        raise ValueError(f"{where}: descriptors are [n_frames][cap][{DESC_LEN}]")
    if d.dtype != np.int16:
        d16 = d.astype(np.int16)
        if not np.array_equal(d16, d):
            raise ValueError(f"{where}: descriptors must be integers of 16 bits")
        d = d16
    n = _i32(n).reshape(-1)
    if len(n) != d.shape[0]:
        raise ValueError(f"{where}: one count per frame")
    return np.ascontiguousarray(d), n


def _sig(where, sig):
    sig = np.ascontiguousarray(sig, np.uint8)
    bits = int(sig.shape[1]).bit_length() - 1 if sig.ndim == 2 else -1
    if sig.ndim != 2 or sig.shape[1] != 1 << bits:
        raise ValueError(f"{where}: signatures are uint8 [n][2^bits]")
    return sig, bits


def _pairs(pairs):
    return _i32(np.reshape(pairs, (-1, 2)))


def place_signatures(desc, n, seed=1, bits=10, ctx=None):
    """viso_place_signatures: uint8 [nf][1 << bits], the hashed bag of words of every frame's first n[f] left-image rows."""
    desc, n = _rows16("place_signatures", desc, n)
    out = np.zeros((len(n), 1 << int(bits)) if 0 <= int(bits) <= 16 else (len(n), 1), np.uint8)
    _call(load().viso_place_signatures, _ctx_h(ctx), ptr(desc, C.c_int16), ptr(n, C.c_int32), len(n), desc.shape[1], int(seed), int(bits),
          ptr(out, C.c_uint8))
    return out


def batch_place_signatures(batch, t0=0, t1=None, seed=1, bits=10):
    """viso_batch_place_signatures: the signatures of frames t0 .. t1-1 (t1 None: to the last) from the rows of the batch's last run."""
    t1 = batch.nf if t1 is None else int(t1)
    out = np.zeros((max(t1 - int(t0), 0), 1 << int(bits)) if 0 <= int(bits) <= 16 else (1, 1), np.uint8)
    _call(load().viso_batch_place_signatures, batch.h, int(t0), t1, int(seed), int(bits), ptr(out, C.c_uint8))
    return out


def place_scores(sig, j0=0, ctx=None):
    """viso_place_scores: uint32 [n - j0][n], row j - j0 = sum_w min(h_j, h_i) for i <= j, 0 for i > j."""
    sig, bits = _sig("place_scores", sig)
    n = len(sig)
    rows = max(n - int(j0), 0)
    # (a block the library refuses is not allocated here first: the call gets a word and answers VISO_ERR_NOMEM)
    out = np.zeros((rows, n) if rows * n * 4 <= 1 << 31 else (1, 1), np.uint32)
    _call(load().viso_place_scores, _ctx_h(ctx), ptr(sig, C.c_uint8), n, bits, int(j0), ptr(out, C.c_uint32))
    return out


def place_candidates(sig, j0=0, min_gap=50, seq_len=1, nms=4, min_score=0, k=4, ctx=None):
    """viso_place_candidates: (cand int32 [n - j0][k] filled with -1, score uint32 [n - j0][k]) of frames j0 .. n-1."""
    sig, bits = _sig("place_candidates", sig)
    if not 0 <= int(min_score) < 1 << 32:
        raise ValueError("place_candidates: min_score is a uint32")
    n, kk = len(sig), max(int(k), 1)
    cand = np.full((max(n - int(j0), 0), kk), -1, np.int32)
    score = np.zeros(cand.shape, np.uint32)
    _call(load().viso_place_candidates, _ctx_h(ctx), ptr(sig, C.c_uint8), n, bits, int(j0), int(min_gap), int(seq_len), int(nms), int(min_score),
          int(k), ptr(cand, C.c_int32), ptr(score, C.c_uint32))
    return cand, score


def _match_lists(out, m):
    return [out[p, :m[p]].copy() for p in range(len(m))]


def wide_match(desc, n, pairs, ratio=0.8, ctx=None):
    """viso_wide_match: for every pair (query frame, target frame) the accepted rows (q, t, sad), int32 [m][3] in ascending q."""
    desc, n = _rows16("wide_match", desc, n)
    pairs = _pairs(pairs)
    out, m = np.zeros((len(pairs), desc.shape[1], 3), np.int32), np.zeros(len(pairs), np.int32)
    _call(load().viso_wide_match, _ctx_h(ctx), ptr(desc, C.c_int16), ptr(n, C.c_int32), len(n), desc.shape[1], ptr(pairs, C.c_int32), len(pairs),
          float(ratio), ptr(out, C.c_int32), ptr(m, C.c_int32))
    return _match_lists(out, m)


def batch_wide_match(batch, pairs, ratio=0.8):
    """viso_batch_wide_match: wide_match between frames of the batch, from the rows of its last run."""
    pairs = _pairs(pairs)
    out, m = np.zeros((len(pairs), batch.cap, 3), np.int32), np.zeros(len(pairs), np.int32)
    _call(load().viso_batch_wide_match, batch.h, ptr(pairs, C.c_int32), len(pairs), float(ratio), ptr(out, C.c_int32), ptr(m, C.c_int32))
    return _match_lists(out, m)


def _stereo_partner(n_left, stereo):
    """right feature of every left feature of a frame's stereo list [m][3] (-1: none)."""
    part = np.full(n_left, -1, np.int64)
    stereo = _i32(stereo).reshape(-1, 3)
    part[stereo[:, 0]] = stereo[:, 1]
    return part


def loop_observations(kp_i, stereo_i, kp_j, stereo_j, matches, param):
    """The solver's inputs for the pair (earlier frame i, later frame j).  kp_* = (left [n][2], right [n][2]) keypoints, stereo_* the
    frame's stereo list [m][3] (Batch.matches(0, t)), matches the wide-match rows of the pair (j, i): (left feature of j, left feature
    of i, sad).  Keeps the rows whose two left features both have a stereo match and returns (X [3][M]: frame i's triangulation,
    obs [4][M]: frame j's uL vL uR vR, the kept rows [M][3])."""
    kpLi, kpRi = (_f32(a).reshape(-1, 2) for a in kp_i)
    kpLj, kpRj = (_f32(a).reshape(-1, 2) for a in kp_j)
    matches = _i32(matches).reshape(-1, 3)
    pi, pj = _stereo_partner(len(kpLi), stereo_i), _stereo_partner(len(kpLj), stereo_j)
    keep = (pj[matches[:, 0]] >= 0) & (pi[matches[:, 1]] >= 0)
    rows = matches[keep]
    zero = np.zeros(len(rows), np.int64)
    X = triangulate_rectified(collect_matches(kpLi, kpRi, np.stack([rows[:, 1], pi[rows[:, 1]], zero], 1)), param)
    obs = collect_matches(kpLj, kpRj, np.stack([rows[:, 0], pj[rows[:, 0]], zero], 1))
    return X, obs, rows


def loop_edge(X, obs, param, min_inliers=20, seed=0, frame=0, sigma=None):
    """The edge of one verified revisit: ransac_minimize_reproj over (X, obs), pose_covariance of its inliers (sigma None: estimated)
    and posegraph.motion_edge.  tr maps frame i's points into frame j, as an odometry edge (k - 1, k) does, so the result is the
    edge (node(i), node(j), Z, info).  Returns (Z, info, record) with record = dict(tr, inliers, cov: the covariance record), or
    None when the solve fails, fewer than min_inliers support it, or the covariance's status is not 1."""
    if X.shape[1] < 3:
        return None
    ok, tr, inl = ransac_minimize_reproj(X, obs, param, seed=seed, frame=frame)
    if ok != 1 or len(inl) < min_inliers:
        return None
    rec = pose_covariance(X, obs, tr, inl, param, mode=1 if sigma is None else 2, sigma=sigma)
    if int(rec["status"]) != 1:
        return None
    Z, info = motion_edge(tr, rec["cov"])
    return Z, info, dict(tr=tr, inliers=inl, cov=rec)


def frame_nodes(ok):
    """The node of every frame in hostmath.chain_poses' list (frame 0 is node 0, every later frame with ok != 0 pushes the next
    pose); -1 for a frame that pushed none."""
    ok = np.asarray(ok).reshape(-1)
    nodes = np.full(len(ok), -1, np.int64)
    k = 0
    for t in range(len(ok)):
        if t == 0:
            nodes[t] = 0
        elif ok[t]:
            k += 1
            nodes[t] = k
    return nodes


def detect_loops(batch, param, seed=1, bits=10, min_gap=50, seq_len=1, nms=4, min_score=0, k=4, ratio=0.8, min_inliers=20,
                 ransac_seed=0, sigma=None, details=None):
    """Loop edges among the frames of one batch, after a run: signatures of the resident rows, candidates, the batch wide match of
    every (frame, candidate) pair and loop_edge of its matches.  Returns [(frame_i, frame_j, Z, info, n_inl)], i < j, FRAME indices
    (frame_nodes gives the nodes).  details: a dict that receives sig, cand, score, pairs and matches.  Call it before the next
    upload: the device calls read the last run's rows and counts, the keypoints come from the getters, which serve the upload's."""
    sig = batch_place_signatures(batch, seed=seed, bits=bits)
    cand, score = place_candidates(sig, min_gap=min_gap, seq_len=seq_len, nms=nms, min_score=min_score, k=k, ctx=batch.ctx)
    pairs = [(j, int(i)) for j in range(len(cand)) for i in cand[j] if i >= 0]
    matches = batch_wide_match(batch, pairs, ratio) if pairs else []
    if details is not None:
        details.update(sig=sig, cand=cand, score=score, pairs=pairs, matches=matches)
    frames = {}

    def frame(t):
        if t not in frames:
            frames[t] = ((batch.keypoints(t, 0), batch.keypoints(t, 1)), batch.matches(0, t))
        return frames[t]

    edges = []
    for (j, i), rows in zip(pairs, matches):
        if len(rows) < min_inliers:
            continue
        (kp_i, st_i), (kp_j, st_j) = frame(i), frame(j)
        X, obs, _ = loop_observations(kp_i, st_i, kp_j, st_j, rows, param)
        e = loop_edge(X, obs, param, min_inliers=min_inliers, seed=ransac_seed, frame=j, sigma=sigma)
        if e is not None:
            edges.append((i, j, e[0], e[1], len(e[2]["inliers"])))
    return edges
