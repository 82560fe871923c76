"""The loop-closure detection (include/viso_hip.h, "loop closure") at the size of KITTI sequence 00: place signatures
of 4541 frames x 2000 rows, scores plus candidates over 4541 signatures at bits 10 and 12 and seq_len 1 and 8, and the wide match of
64 and 256 pairs of 2000 x 2000 rows.  Wall times are medians of 7 with min-max; the host clock goes around calls that end in a
synchronise (a direct call's uploads and downloads are inside it).  The yardstick is the numpy restatement (tests/loop_ref.py) on the
host for the same inputs; where that would take minutes it runs a stated share of the work and the row says `host_share`.

    python tools/loop_bench.py [--frames N] [--rows R] [--repeat K] [--no-host] [--legs sig cand wide]
    python tools/loop_bench.py --kernel-only        # one call of every leg: the run to put under rocprofv3 --kernel-trace --stats

One JSON line a row.  The restatement is test code, read from here."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from libviso_amd import loops, synth  # noqa: E402
import loop_ref as LR  # noqa: E402


def timed(fn, repeat):
    fn()   # warm: the first call loads the code object and grows the scratch blocks
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t)), out


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def frames_of(rng, distinct, rows):
    """`distinct` frames of `rows` synthetic descriptors, each frame a noisy view of one pool (so that signatures and matches are not empty)."""
    pool = synth._new_desc(rng, rows)
    out = np.empty((distinct, rows, 121), np.int16)
    for f in range(distinct):
        out[f] = np.clip(pool[rng.permutation(rows)] + np.rint(rng.normal(0, 6.0, (rows, 121))), -1020, 1020)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=4541)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--seed", type=int, default=4541)
    ap.add_argument("--no-host", action="store_true", help="leave the numpy yardstick out")
    ap.add_argument("--kernel-only", action="store_true", help="one call per leg and nothing else")
    ap.add_argument("--legs", nargs="+", default=["sig", "cand", "wide"])
    a = ap.parse_args(argv)
    rng = np.random.default_rng(a.seed)
    rep = 1 if a.kernel_only else a.repeat

    if "sig" in a.legs:
        distinct = min(a.frames, 32)
        desc = np.tile(frames_of(rng, distinct, a.rows), ((a.frames + distinct - 1) // distinct, 1, 1))[:a.frames]
        n = np.full(a.frames, a.rows, np.int32)
        for bits in (10, 12):
            if a.kernel_only:
                loops.place_signatures(desc, n, seed=1, bits=bits)
                continue
            t, sig = timed(lambda: loops.place_signatures(desc, n, seed=1, bits=bits), rep)
            row = dict(leg="place_signatures", frames=a.frames, rows=a.rows, bits=bits, upload_bytes=int(desc.nbytes), call=t)
            if not a.no_host:
                ms, want = host_ms(lambda: LR.signatures(desc[:distinct], n[:distinct], 1, bits))
                assert np.array_equal(want, sig[:distinct])
                row["host"] = dict(ms=ms * a.frames / distinct, host_share=distinct / a.frames)
            print(json.dumps(row), flush=True)
        del desc

    if "cand" in a.legs:
        for bits in (10, 12):
            # signatures like a sequence's: 2000 rows a frame over 2^bits words, neighbouring frames alike
            base = rng.poisson(a.rows / (1 << bits), (a.frames // 8 + 2, 1 << bits))
            sig = np.minimum(np.repeat(base, 8, 0)[:a.frames] + rng.poisson(0.3, (a.frames, 1 << bits)), 255).astype(np.uint8)
            for seq_len in (1, 8):
                kw = dict(min_gap=50, seq_len=seq_len, nms=4, k=4)
                if a.kernel_only:
                    loops.place_candidates(sig, **kw)
                    continue
                t, (cand, score) = timed(lambda: loops.place_candidates(sig, **kw), rep)
                row = dict(leg="place_candidates", n=a.frames, bits=bits, seq_len=seq_len, cells=a.frames * (a.frames + 1) // 2, call=t)
                if not a.no_host and seq_len == 1:
                    j0 = a.frames - max(a.frames // 64, 1)            # the last rows: each against all frames before it
                    ms, _ = host_ms(lambda: LR.scores(sig, j0))
                    share = sum(range(j0 + 1, a.frames + 1)) / (a.frames * (a.frames + 1) / 2)
                    row["host"] = dict(scores_ms=ms / share, host_share=share)
                print(json.dumps(row), flush=True)

    if "wide" in a.legs:
        nf = 16
        desc = frames_of(rng, nf, a.rows)
        n = np.full(nf, a.rows, np.int32)
        for np_ in (64, 256):
            pairs = [(p % nf, (p * 5 + 1 + p // nf) % nf) for p in range(np_)]
            if a.kernel_only:
                loops.wide_match(desc, n, pairs, 0.8)
                continue
            t, m = timed(lambda: loops.wide_match(desc, n, pairs, 0.8), rep)
            row = dict(leg="wide_match", pairs=np_, rows=a.rows, cells=np_ * a.rows * a.rows, matches=int(sum(len(x) for x in m)), call=t)
            if not a.no_host:
                ms, want = host_ms(lambda: LR.wide_match(desc, n, pairs[:2], 0.8))
                assert all(np.array_equal(x, y) for x, y in zip(want, m[:2]))
                row["host"] = dict(ms=ms * np_ / 2, host_share=2 / np_)
            print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
