"""Cost of an opt-in motion estimator at configs[2] size: 512 frame pairs (513 frames), 2000 keypoints per image, the end-to-end step
(matcher + circle join + RANSAC/Gauss-Newton) with the estimator off and on.

  python tools/estimator_bench.py {covariance,refine,window} [--K K] [--steps N] [--regions R] [--out FILE]

covariance: viso_batch_set_covariance, mode 0 against mode 1 (motion_cov_kernel).  refine: viso_batch_set_refine, mode 0 against
mode 1 (motion_refine_kernel).  window: viso_batch_set_window_refine, off against K (default 4; window_links_kernel,
window_refine_kernel).

Two batches over the same frames, one off and one on, in one process; timed regions of N steps each (host clock around N runs that
end in a synchronise and the poses' read-back), alternating between the two; the median region of each is reported.  The kernels'
own times come from a separate run under `rocprofv3 --kernel-trace --stats`, e.g. with --regions 1 --steps 3."""
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


def _status1(recs):
    return recs[recs["status"] == 1]


# per stage: the setter (batch, on), the records getter, what the timings are called, and the stage's own figures of the records
STAGES = {
    "covariance": dict(
        set=lambda b, on, K: b.set_covariance(int(on)), records=lambda b: b.covariances(), keys=("mode0", "mode1"),
        what=lambda K: "mode 0 vs mode 1", changed="mode 1 changed the poses",
        figures=lambda recs: {"median_inliers": float(np.median(recs["n"][1:]))}),
    "refine": dict(
        set=lambda b, on, K: b.set_refine(int(on)), records=lambda b: b.refines(), keys=("mode0", "mode1"),
        what=lambda K: "mode 0 vs mode 1", changed="mode 1 changed the poses",
        figures=lambda recs: {"median_points": float(np.median(recs["n"][1:])),
                              "iters_mean": float(_status1(recs)["iters"].mean()),
                              "iters_hist": np.bincount(_status1(recs)["iters"]).tolist()}),
    "window": dict(
        set=lambda b, on, K: b.set_window_refine(K if on else 0), records=lambda b: b.window_refines(), keys=("off", "on"),
        what=lambda K: f"window off vs K = {K}", changed="the window changed the poses",
        figures=lambda recs: {"median_points": float(np.median(recs["n_points"][1:])),
                              "median_rows": float(np.median(recs["n_rows"][1:])),
                              "mean_len": float(_status1(recs)["len"].mean()),
                              "iters_mean": float(_status1(recs)["iters"].mean()),
                              "iters_hist": np.bincount(_status1(recs)["iters"]).tolist()}),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("stage", choices=sorted(STAGES))
    ap.add_argument("--frames", type=int, default=513)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--K", type=int, default=4, help="window size (window only)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    st_ = STAGES[a.stage]
    seq = synth.make_sequence(2000, 33, n_kp=a.kp)
    rep = lambda x: np.ascontiguousarray(np.resize(x, (a.frames,) + x.shape[1:]))   # noqa: E731
    kp, desc, n = rep(seq["kp"]), rep(seq["desc"]), rep(seq["n"])
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    ctx = libviso_amd.Context(0)
    batches = {}
    for on in (0, 1):
        b = libviso_amd.Batch(ctx, a.frames, a.kp)
        b.upload(kp, desc, n)
        b.set_params(st, tm, seq["param"], seed=1)
        st_["set"](b, on, a.K)
        batches[on] = b

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
        for on in (0, 1):
            times[on].append(region(batches[on]))
    p0, p1 = batches[0].poses(), batches[1].poses()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(p0, p1)), st_["changed"]
    recs = st_["records"](batches[1])
    med = {on: float(np.median(times[on])) / a.steps * 1e3 for on in (0, 1)}
    k0, k1 = st_["keys"]
    res = {"workload": f"configs[2] end-to-end step, {a.frames - 1} pairs x {a.kp} kp, {st_['what'](a.K)} alternated"}
    if a.stage == "window":
        res["K"] = a.K
    res.update({f"ms_per_step_{k0}": med[0], f"ms_per_step_{k1}": med[1],
                "overhead_pct": 100.0 * (med[1] - med[0]) / med[0],
                "regions": a.regions, "steps_per_region": a.steps,
                "spread_ms_per_step": {str(on): [float(np.min(times[on])) / a.steps * 1e3, float(np.max(times[on])) / a.steps * 1e3]
                                       for on in (0, 1)},
                "frames_status1": int((recs["status"] == 1).sum())})
    res.update(st_["figures"](recs))
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
