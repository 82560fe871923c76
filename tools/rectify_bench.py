"""Cost of the opt-in rectification (viso_batch_set_rectify) at configs[1] batch size: 513 stereo frames of KITTI-raw geometry
1392x512 rectified to 1241x376, 2000 keypoints per image.

  python tools/rectify_bench.py [--reps N] [--out FILE]

Legs (host clock, median of alternating repetitions):
  remap_only         viso_batch_upload_images of raw frames already in pinned memory, minus the same upload with rectification
                     off (the raw copy is larger: that difference is reported too); run under
                     `rocprofv3 --kernel-trace --stats` for the kernel's own time;
  step_resident      run_images on resident images (rectification plays no part there: the baseline step);
  stream_rectified / stream_raw_rectified
                     every step uploads fresh images asynchronously from pinned memory and runs the pipeline: rectified images
                     (rectification off) vs raw images (rectification on).
The frames are 17 synthetic frames (synth.make_image_sequence, rendered raw by synth.distort_image_sequence) repeated."""
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
    ap.add_argument("--frames", type=int, default=513)
    ap.add_argument("--kp", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nf = a.frames
    seq = synth.make_image_sequence(2000, 17, n_kp=a.kp)
    calib = synth.raw_stereo_calib(0)
    d = synth.distort_image_sequence(seq, calib, seed=1)
    rep = lambda x: np.ascontiguousarray(np.resize(x, (nf,) + x.shape[1:]))   # noqa: E731
    rect, raw, kp, n = rep(seq["images"]), rep(d["images"]), rep(seq["kp"]), rep(seq["n"])
    maps = [libviso_amd.rectify_map(calib["K"][s], calib["D"][s], calib["R"][s], calib["P"][s], calib["out_shape"]) for s in (0, 1)]
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    ctx = libviso_amd.Context(0)
    bo = libviso_amd.Batch(ctx, nf, a.kp)   # rectification off
    br = libviso_amd.Batch(ctx, nf, a.kp)   # rectification on
    br.set_rectify(calib["raw_shape"], calib["out_shape"], left=maps[0], right=maps[1])
    pr, praw, pk = (libviso_amd.PinnedArray(x.shape, x.dtype) for x in (rect, raw, kp))
    pr.a[...] = rect; praw.a[...] = raw; pk.a[...] = kp
    for b in (bo, br):
        b.set_params(st, tm, seq["param"], seed=1)
    bo.upload_images(pr.a, pk.a, n)
    br.upload_images(praw.a, pk.a, n)
    assert np.array_equal(br.image(0, 0), libviso_amd.rectify_images(raw[0, 0], maps[0][0], maps[0][1], calib["out_shape"]))

    def clock(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return time.perf_counter() - t0

    legs = {k: [] for k in ("upload_rectified", "upload_raw_rectify", "step_resident", "stream_rectified", "stream_raw_rectified")}
    for _ in range(2):   # warm-up
        bo.run_images(); br.run_images()
    for i in range(a.reps):   # alternating
        legs["upload_rectified"].append(clock(lambda: bo.upload_images(pr.a, pk.a, n)))
        legs["upload_raw_rectify"].append(clock(lambda: br.upload_images(praw.a, pk.a, n)))
        legs["step_resident"].append(clock(lambda: bo.run_images()))
        legs["stream_rectified"].append(clock(lambda: (bo.upload_images_async(pr.a, pk.a, n), bo.run_images())))
        legs["stream_raw_rectified"].append(clock(lambda: (br.upload_images_async(praw.a, pk.a, n), br.run_images())))
    med = {k: float(np.median(v)) * 1e3 for k, v in legs.items()}
    res = {"frames_per_step": nf, "images_per_step": 2 * nf, "raw_shape": list(calib["raw_shape"]), "out_shape": list(calib["out_shape"]),
           "ms_median": med, "ms_min": {k: float(np.min(v)) * 1e3 for k, v in legs.items()},
           "fps_stream_rectified": (nf - 1) / med["stream_rectified"] * 1e3,
           "fps_stream_raw_rectified": (nf - 1) / med["stream_raw_rectified"] * 1e3,
           "bytes": {"raw": int(raw.nbytes), "rectified": int(rect.nbytes), "maps": 2 * 8 * int(np.prod(calib["out_shape"]))}}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    for x in (pr, praw, pk):
        x.close()
    bo.close(); br.close(); ctx.close()


if __name__ == "__main__":
    main()
