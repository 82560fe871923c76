"""The oracle at bench size: oracle.sequence over contiguous chunks and the per-call match lists, on a thread pool.

oracle_sequence carries one frame of state (the previous stereo list and its 3-D points, src/viso.cpp:1208-1222) and
keys RANSAC by first_frame + t.  A chunk that starts one frame early (the halo) and passes first_frame + its own start
therefore computes exactly what one whole call computes for its frames; the halo frame's own outputs are dropped.
ctypes releases the GIL around the C calls, so threads run the chunks in parallel.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import pyoracle as oracle

MAX_WORKERS = 16        # a GPU machine's command gets 16 CPUs, whatever os.cpu_count() says


def _pool(workers):
    return ThreadPoolExecutor(max_workers=max(1, min(int(workers), MAX_WORKERS)))


def sequence_chunked(kp, desc, n, st, tm, param, seed=0, first_frame=0, workers=MAX_WORKERS, chunk=None,
                     matcher_only=False):
    """oracle.sequence(kp, desc, n, ...) computed chunk by chunk: the same dict of tr, ok, n_inl, scored, m_out."""
    nf = kp.shape[0]
    workers = max(1, min(int(workers), MAX_WORKERS))
    chunk = chunk or max(2, -(-nf // (2 * workers)))
    starts = list(range(0, nf, chunk))

    def one(s):
        lo, hi = max(0, s - 1), min(nf, s + chunk)
        r = oracle.sequence(kp[lo:hi], desc[lo:hi], n[lo:hi], st, tm, param, seed=seed, first_frame=first_frame + lo,
                            matcher_only=matcher_only)
        k = s - lo                                  # the halo frame, if any, is dropped
        return s, {key: (v[:, k:] if key in ("scored", "m_out") else v[k:]) for key, v in r.items() if key != "stage_s"}

    with _pool(workers) as ex:
        parts = dict(ex.map(one, starts))
    out = {}
    for key in ("tr", "ok", "n_inl"):
        out[key] = np.concatenate([parts[s][key] for s in starts], 0)
    for key in ("scored", "m_out"):
        out[key] = np.concatenate([parts[s][key] for s in starts], 1)
    return out


def pair(which, t):
    """(query, target) as (side, frame) of match kind `which` at frame t: 0 stereo, 1 temporal left, 2 temporal right."""
    q = (0, t) if which < 2 else (1, t)
    tg = (1, t) if which == 0 else ((0, t - 1) if which == 1 else (1, t - 1))
    return q, tg


def match_one(seq, which, t, st, tm):
    """The oracle's match list and scored-pair count of one call."""
    kp, desc, n = seq["kp"], seq["desc"], seq["n"]
    (qs, qf), (ts, tf) = pair(which, t)
    nq, nt = n[qf, qs], n[tf, ts]
    return oracle.match_desc(kp[qf, qs, :nq], kp[tf, ts, :nt], desc[qf, qs, :nq], desc[tf, ts, :nt],
                             st if which == 0 else tm, return_scored=True)


def lists(seq, frames, kinds, st, tm, workers=MAX_WORKERS):
    """{(which, t): (matches, scored)} of the oracle for every t in frames and which in kinds (temporal kinds from t = 1)."""
    keys = [(w, int(t)) for t in frames for w in kinds if w == 0 or t >= 1]
    with _pool(workers) as ex:
        res = list(ex.map(lambda k: match_one(seq, k[0], k[1], st, tm), keys))
    return dict(zip(keys, res))
