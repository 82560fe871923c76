"""Cost of the opt-in voxel map (viso_map_*, viso_batch_fuse_disparities) at 512 block-matching maps of 1241x376, default
parameters (voxel 0.2 m, min_disp16 16, 2^24 slots; the next capacity that holds the scene when that one overflows).

  python tools/map_bench.py [--frames N] [--reps N] [--host-frames N] [--capacity-log2 N] [--kernel-only] [--out FILE]

The pairs are 17 seeded synthetic frames (synth.make_image_sequence: textured patches) repeated; frame t gets the pose of a camera
that has moved 0.8 t m forward and turned 0.002 t rad, so that the frames overlap as a drive's do.  Legs (host clock around work
that ends in a synchronise, medians of alternating repetitions):
  fuse      Batch.fuse_disparities of all resident maps into a cleared map (the clear is outside the clock);
  extract   VoxelMap.entries(): two compaction passes, the copy of the entries, the sort on the host;
  direct    one viso_map_fuse call of one host map (copy in, one kernel);
  clear     viso_map_clear.
  host      what a user has without the map, on --host-frames of the same maps: Batch.disparity_points per frame (kernel and 5.6 MB
            copy), then floor(P / voxel) and np.unique with counts per frame, and one np.unique over the frames' voxels at the end.
            Reported per frame.
n_inserts / n_points from viso_map_stats is what the combining inside the waves buys.  --kernel-only runs clear + fuse --reps
times and extraction once: the run to put under `rocprofv3 --kernel-trace --stats` for the kernels' own times.  The count the
result is held against (not a measurement) is printed with it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import libviso_amd  # noqa: E402
from libviso_amd import hostmath, synth  # noqa: E402
from libviso_amd.abi import MatchParams  # noqa: E402


def count_ms(nf, rows, cols):
    """A count, not a measurement: every map read once (2 B a pixel) over 8 TB/s.  A floor for the pass: the table's atomics are
    not in it."""
    b = float(rows) * cols * nf * 2
    return b, b / 8e12 * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-frames", type=int, default=16)
    ap.add_argument("--capacity-log2", type=int, default=24)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nf = a.frames
    seq = synth.make_image_sequence(2000, 17, n_kp=64)
    images = np.ascontiguousarray(np.resize(seq["images"], (nf,) + seq["images"].shape[1:]))
    rows, cols = images.shape[2:]
    poses = np.array([np.linalg.inv(hostmath.tr2mat([0.0, 0.002 * t, 0.0, 0.0, 0.0, -0.8 * t])) for t in range(nf)])
    ctx = libviso_amd.Context(0)

    def clock(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    b = libviso_amd.Batch(ctx, nf, 64)
    b.upload_images_only(images)
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"])
    b.set_disparity({})
    b.run_disparity()
    # the default capacity, or the next one that holds the scene (the result names the one used)
    for log2 in (a.capacity_log2, 26, 28):
        vmap = libviso_amd.VoxelMap(ctx, capacity_log2=log2)
        try:
            b.fuse_disparities(vmap, poses)
            break
        except libviso_amd.VisoError as e:
            vmap.close()
            if "-4" not in str(e) or log2 == 28:
                raise
    voxel = vmap.voxel

    if a.kernel_only:
        ms = []
        for _ in range(a.reps):
            vmap.clear()
            ms.append(clock(lambda: b.fuse_disparities(vmap, poses)))
        n = len(vmap.entries())
        print(json.dumps({"frames": nf, "fuse_ms": ms, "voxels": n}))
        vmap.close(); b.close(); ctx.close()
        return

    one = libviso_amd.VoxelMap(ctx, capacity_log2=log2)
    map0 = b.disparity(0)
    for _ in range(2):   # warm-up
        vmap.clear(); b.fuse_disparities(vmap, poses); vmap.entries()
        one.clear(); one.fuse(map0, seq["param"], pose=poses[0])
    legs = {k: [] for k in ("fuse", "extract", "direct", "clear")}
    for _ in range(a.reps):   # alternating
        legs["clear"].append(clock(vmap.clear))
        legs["fuse"].append(clock(lambda: b.fuse_disparities(vmap, poses)))
        legs["extract"].append(clock(vmap.entries))
        one.clear()
        legs["direct"].append(clock(lambda: one.fuse(map0, seq["param"], pose=poses[0])))
    entries, st = vmap.entries(), vmap.stats()

    # the host path on the first frames of the same maps
    hf = min(a.host_frames, nf)
    host_ms, parts = [], []
    for t in range(hf):
        t0 = time.perf_counter()
        P = b.disparity_points(t, pose=poses[t], min_disp16=16)
        P = P[np.isfinite(P[..., 2])].astype(np.float64)
        k = np.floor(P / voxel).astype(np.int64) + (1 << 20)
        keys, cnt = np.unique((k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2], return_counts=True)
        parts.append((keys, cnt))
        host_ms.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    keys, inv = np.unique(np.concatenate([p[0] for p in parts]), return_inverse=True)
    cnt = np.zeros(len(keys), np.int64)
    np.add.at(cnt, inv, np.concatenate([p[1] for p in parts]))
    merge_ms = (time.perf_counter() - t0) * 1e3
    # (the host path rounds P to float32 first, so its voxels can differ from the map's at cell faces; the totals must agree)
    chk = libviso_amd.VoxelMap(ctx, capacity_log2=log2)
    b.fuse_disparities(chk, poses[:hf], t0=0, t1=hf)
    assert int(cnt.sum()) == int(chk.entries()["count"].sum())
    chk.close()

    res = {"frames": nf, "shape": [int(rows), int(cols)], "params": "voxel 0.2, min_disp16 16", "capacity_log2": log2, "reps": a.reps,
           "ms_median": {k: float(np.median(v)) for k, v in legs.items()}, "ms_min": {k: float(np.min(v)) for k, v in legs.items()},
           "stats": st, "voxels": int(len(entries)), "inserts_per_point": st["n_inserts"] / max(1, st["n_points"]),
           "host": {"frames": hf, "ms_per_frame_median": float(np.median(host_ms)), "merge_ms": merge_ms, "voxels": int(len(keys))}}
    res["count_bytes"], res["count_ms"] = count_ms(nf, rows, cols)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    for v in (vmap, one):
        v.close()
    b.close(); ctx.close()


if __name__ == "__main__":
    main()
