"""Cost of the opt-in sliding-window bundle adjustment (viso_batch_set_window_refine) at configs[2] size: 512 frame pairs (513 frames),
2000 keypoints per image, the end-to-end step (matcher + circle join + RANSAC/Gauss-Newton) with the window off and with window K.

  python tools/window_bench.py [--K K] [--steps N] [--regions R] [--out FILE]

Two batches over the same frames, one off and one with K, in one process; timed regions of N steps each (host clock around N runs
that end in a synchronise and the poses' read-back), alternating between the two; the median region of each is reported.  The
kernels' own times (window_links_kernel, window_refine_kernel) come from a separate run under `rocprofv3 --kernel-trace --stats`,
e.g. with --regions 1 --steps 3 for each K."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libviso_amd  # noqa: E402
from libviso_amd import synth  # noqa: E402
from libviso_amd.abi import MatchParams  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--frames", type=int, default=513)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    seq = synth.make_sequence(2000, 33, n_kp=a.kp)
    rep = lambda x: np.ascontiguousarray(np.resize(x, (a.frames,) + x.shape[1:]))   # noqa: E731
    kp, desc, n = rep(seq["kp"]), rep(seq["desc"]), rep(seq["n"])
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    ctx = libviso_amd.Context(0)
    batches = {}
    for mode in (0, 1):
        b = libviso_amd.Batch(ctx, a.frames, a.kp)
        b.upload(kp, desc, n)
        b.set_params(st, tm, seq["param"], seed=1)
        b.set_window_refine(a.K if mode else 0)
        batches[mode] = b

    def region(b):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            b.run()
        b.poses()
        return time.perf_counter() - t0

    for b in batches.values():   # warm-up: code objects, buffers
        region(b)
    times = {0: [], 1: []}
    for _ in range(a.regions):
        for mode in (0, 1):
            times[mode].append(region(batches[mode]))
    p0, p1 = batches[0].poses(), batches[1].poses()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(p0, p1)), "the window changed the poses"
    recs = batches[1].window_refines()
    med = {m: float(np.median(times[m])) / a.steps * 1e3 for m in (0, 1)}
    res = {"workload": f"configs[2] end-to-end step, {a.frames - 1} pairs x {a.kp} kp, window off vs K = {a.K} alternated",
           "K": a.K, "ms_per_step_off": med[0], "ms_per_step_on": med[1],
           "overhead_pct": 100.0 * (med[1] - med[0]) / med[0],
           "regions": a.regions, "steps_per_region": a.steps,
           "spread_ms_per_step": {str(m): [float(np.min(times[m])) / a.steps * 1e3, float(np.max(times[m])) / a.steps * 1e3]
                                  for m in (0, 1)},
           "frames_status1": int((recs["status"] == 1).sum()), "median_points": float(np.median(recs["n_points"][1:])),
           "median_rows": float(np.median(recs["n_rows"][1:])), "mean_len": float(recs["len"][recs["status"] == 1].mean()),
           "iters_mean": float(recs["iters"][recs["status"] == 1].mean()),
           "iters_hist": np.bincount(recs["iters"][recs["status"] == 1]).tolist()}
    for b in batches.values():
        b.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
