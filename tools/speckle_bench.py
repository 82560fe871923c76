"""Cost of the opt-in speckle filter (viso_batch_set_speckle) at 512 stereo frames of 1241x376, default parameters.

  python tools/speckle_bench.py [--frames N] [--reps N] [--methods bm,sgm] [--kernel-only] [--out FILE]

The pairs are 17 seeded synthetic frames (synth.make_image_sequence: textured patches) repeated.  Legs (host clock around work
that ends in a synchronise, median of alternating repetitions), for each method:
  dense_off / dense_on   run_disparity on resident images with the filter off / on (two batches of the same frames): the dense
                         stage as a user pays for it.  The filter's own time is far below the spread of either leg: take it from
                         the kernel trace (--kernel-only);
  direct_*               one viso_filter_speckles call (copy in, four kernels, copy out) of one map: a real one (the method's map
                         of frame 0), the constant map (one root takes every count) and the one-pixel serpentine (the deepest
                         union-find trees): the input dependence of the filter.
--kernel-only runs just run_disparity with block matching and the filter on --reps times: the run to put under
`rocprofv3 --kernel-trace --stats` for the kernels' own times; with --input real|constant|serpentine it runs --reps direct calls
on that one map instead (the input dependence, kernel by kernel).  The count they are priced against (not a measurement) is printed
with the result."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import libviso_amd  # noqa: E402
from libviso_amd import synth  # noqa: E402
from speckle_ref import serpentine  # noqa: E402

TOUCHES = 4   # times the 8 bytes of workspace per pixel move: written by the tile kernel, read and written by the count kernel, read by the removal


def count_ms(nf, rows, cols):
    """A count, not a measurement: the map read twice and written once at worst (2 B each), the workspace's 8 B TOUCHES / 2 times,
    over 8 TB/s."""
    b = float(rows) * cols * nf * (3 * 2 + 8 * TOUCHES / 2)
    return b, b / 8e12 * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--methods", default="bm,sgm")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--input", default=None, choices=("real", "constant", "serpentine"),
                    help="with --kernel-only: --reps direct calls on this one map instead of the batch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nf = a.frames
    seq = synth.make_image_sequence(2000, 17, n_kp=64)
    images = np.ascontiguousarray(np.resize(seq["images"], (nf,) + seq["images"].shape[1:]))
    rows, cols = images.shape[2:]
    ctx = libviso_amd.Context(0)

    def clock(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def batch(method, speckle):
        b = libviso_amd.Batch(ctx, nf, 64)
        b.upload_images_only(images)
        (b.set_disparity if method == "bm" else b.set_sgm)({})
        if speckle:
            b.set_speckle({})
        return b

    if a.kernel_only and a.input:
        m = {"real": lambda: libviso_amd.stereo_disparity(images[0, 0], images[0, 1]), "constant": lambda: np.full((rows, cols), 320, np.int16),
             "serpentine": lambda: serpentine(rows, cols)[0]}[a.input]()
        ms = [clock(lambda: libviso_amd.filter_speckles(m)) for _ in range(a.reps)]
        print(json.dumps({"input": a.input, "direct_ms": ms}))
        ctx.close()
        return
    if a.kernel_only:
        b = batch("bm", True)
        ms = [clock(b.run_disparity) for _ in range(a.reps)]
        print(json.dumps({"frames": nf, "dense_on_ms": ms}))
        b.close(); ctx.close()
        return

    res = {"frames": nf, "shape": [int(rows), int(cols)], "params": "defaults (max_size 100, max_diff 16)", "reps": a.reps, "methods": {}}
    shapes = {"constant": np.full((rows, cols), 320, np.int16), "serpentine": serpentine(rows, cols)[0]}
    for method in a.methods.split(","):
        bo, bd = batch(method, False), batch(method, True)
        for _ in range(2):   # warm-up
            bo.run_disparity(); bd.run_disparity()
        real = bo.disparity(0)
        maps = dict(shapes, real=real)
        for m in maps.values():
            libviso_amd.filter_speckles(m)
        legs = {k: [] for k in ["dense_off", "dense_on"] + ["direct_" + k for k in maps]}
        for _ in range(a.reps):   # alternating
            legs["dense_off"].append(clock(bo.run_disparity))
            legs["dense_on"].append(clock(bd.run_disparity))
            for k, m in maps.items():
                legs["direct_" + k].append(clock(lambda m=m: libviso_amd.filter_speckles(m)))
        assert np.array_equal(bd.disparity(3), libviso_amd.filter_speckles(bo.disparity(3)))
        med = {k: float(np.median(v)) for k, v in legs.items()}
        res["methods"][method] = {"ms_median": med, "ms_min": {k: float(np.min(v)) for k, v in legs.items()},
                                  "valid_share_frame0": [float((real != -16).mean()), float((bd.disparity(0) != -16).mean())]}
        bo.close(); bd.close()
    res["count_bytes"], res["count_ms"] = count_ms(nf, rows, cols)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
