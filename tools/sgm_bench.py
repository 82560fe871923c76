"""Cost of the opt-in semi-global matching (viso_batch_set_sgm) at 512 stereo frames of 1241x376, default parameters.

  python tools/sgm_bench.py [--frames N] [--reps N] [--kernel-only] [--out FILE]

The pairs are 17 seeded synthetic frames (synth.make_image_sequence: textured patches, 2000 keypoints per image) repeated.
Legs (host clock around work that ends in a synchronise, median of alternating repetitions):
  step_off / step_on   run_images on resident images with SGM off / on (two batches of the same frames);
  disparity_only       run_disparity: the SGM kernels alone over every frame of the batch (in workspace groups);
  direct_call          one viso_stereo_sgm call (copy in, kernels, copy out) of one pair.
--kernel-only runs just run_disparity --reps times: the run to put under `rocprofv3 --kernel-trace --stats` for the kernels' own
time.  The floor they are priced against (a count, not a measurement) is printed with the result."""
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


UPDATE_OPS = 20   # VALU lane-operations of sgm_path_kernel per (pixel, d, path): cost 4 (xor, bcnt), recursion 9, S packing and add 7


def floor_ms(nf, rows, cols, D=128, paths=8):
    """Two counts, not measurements.  Bytes of S traffic (2 bytes per (pixel, d): written once, read and written by the other
    paths - 1 launches, read by the selection) over 8 TB/s; (pixel, d, path) updates at UPDATE_OPS lane-ops against 256 CUs x 64
    lanes x 2.4 GHz."""
    cells = float(rows) * cols * D * nf
    s_bytes = cells * 2 * (1 + 2 * (paths - 1) + 1)
    return s_bytes, s_bytes / 8e12 * 1e3, cells * paths, cells * paths * UPDATE_OPS / (256 * 64 * 2.4e9) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nf = a.frames
    seq = synth.make_image_sequence(2000, 17, n_kp=a.kp)
    rep = lambda x: np.ascontiguousarray(np.resize(x, (nf,) + x.shape[1:]))   # noqa: E731
    images, kp, n = rep(seq["images"]), rep(seq["kp"]), rep(seq["n"])
    rows, cols = images.shape[2:]
    ctx = libviso_amd.Context(0)

    def clock(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    if a.kernel_only:
        b = libviso_amd.Batch(ctx, nf, 64)
        b.upload_images_only(images)
        b.set_sgm({})
        ms = [clock(b.run_disparity) for _ in range(a.reps)]
        print(json.dumps({"frames": nf, "disparity_only_ms": ms}))
        b.close(); ctx.close()
        return

    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    bo = libviso_amd.Batch(ctx, nf, a.kp)   # SGM off
    bd = libviso_amd.Batch(ctx, nf, a.kp)   # SGM on
    for b in (bo, bd):
        b.upload_images(images, kp, n)
        b.set_params(st, tm, seq["param"], seed=1)
    bd.set_sgm({})
    for _ in range(2):   # warm-up
        bo.run_images(); bd.run_images(); bd.run_disparity()
    legs = {k: [] for k in ("step_off", "step_on", "disparity_only", "direct_call")}
    for _ in range(a.reps):   # alternating
        legs["step_off"].append(clock(bo.run_images))
        legs["step_on"].append(clock(bd.run_images))
        legs["disparity_only"].append(clock(bd.run_disparity))
        legs["direct_call"].append(clock(lambda: libviso_amd.stereo_sgm(images[0, 0], images[0, 1])))
    assert np.array_equal(bd.disparity(3), libviso_amd.stereo_sgm(images[3, 0], images[3, 1]))
    for got, want in zip(bd.poses(), bo.poses()):
        assert np.array_equal(got, want)
    s_bytes, fl_bytes, updates, fl_valu = floor_ms(nf, rows, cols)
    d0 = bd.disparity(0)
    res = {"frames": nf, "shape": [int(rows), int(cols)], "params": "defaults (D 128, P1 10, P2 120, 8 paths, u 10, m 1)",
           "ms_median": {k: float(np.median(v)) for k, v in legs.items()}, "ms_min": {k: float(np.min(v)) for k, v in legs.items()},
           "reps": a.reps, "s_bytes": s_bytes, "floor_ms_s_traffic_count": fl_bytes, "updates": updates,
           "floor_ms_valu_count": fl_valu, "valid_share_frame0": float((d0 != -16).mean())}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    bo.close(); bd.close(); ctx.close()


if __name__ == "__main__":
    main()
