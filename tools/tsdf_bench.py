"""Cost of the opt-in TSDF map (viso_tsdf_*, viso_batch_fuse_tsdf) at 512 block-matching maps of 1241x376, default parameters
(voxel 0.2 m, T = 3, min_disp16 16, 2^26 slots; the next capacity that holds the scene when that one overflows).

  python tools/tsdf_bench.py [--frames N] [--reps N] [--capacity-log2 N] [--render-views N] [--kernel-only] [--out FILE]
                             [--carve C [--carve-near M]] [--depth-weights S] [--options-capacity-log2 N] [--fuse-only]
                             [--distance-field] [--travel-field] [--retract]

The pairs and poses are those of tools/map_bench.py: 17 seeded synthetic frames repeated, frame t seen from a camera that has moved
0.8 t m forward and turned 0.002 t rad.  Legs (host clock around work that ends in a synchronise, medians of alternating
repetitions):
  fuse_tsdf    Batch.fuse_tsdf of all resident maps into a cleared map (the clear is outside the clock);
  fuse_map     Batch.fuse_disparities of the same maps into a cleared voxel map: the comparison;
  entries      TsdfMap.entries(): two compaction passes, the copy, the sort on the host;
  surface      TsdfMap.surface(): two passes of three probes a voxel, the copy, the sort on the host;
  mesh         TsdfMap.mesh() over the same table: the extraction twice (count, list), each two passes of seven probes a voxel, the
               copies, the two sorts and the resolution of the triangles' references on the host;
  render       TsdfMap.render of --render-views views of the maps' size at fusing poses spread evenly over the sequence, max_depth
               40 m, min_weight 2, one call: the launch, the copy of the views to the host and the free (time per view = / views).
               The marching rate is counted from the result: a pixel with a hit at depth zs has marched ceil(zs / h) samples, one
               without a hit all N = 400;
  clear        viso_tsdf_clear;
  fuse_gray    Batch.fuse_tsdf of the same maps into a cleared gray map (include/viso_hip.h, "TSDF intensity") of the same capacity:
               one more byte read a pixel and three atomics where fuse_tsdf has two per run head;
  vertex_gray  TsdfMap.vertex_gray of the gray map's mesh vertices: the copy up, two probes a vertex, the copy back;
  render_gray  TsdfMap.render(gray=True) of the same views over the gray map: beside `render`, one more 8-byte load a probe and one
               more byte a pixel out.
  render_normals  (include/viso_hip.h, "TSDF normals") TsdfMap.normals.render of the same views over the same map, beside `render`
               in the same loop: the march unchanged, then at most twelve more probes a hit pixel and twelve more bytes a pixel out;
  mesh_normals TsdfMap.normals.mesh() beside `mesh`: the extraction, then the vertices up, at most twelve probes a vertex and
               twelve bytes a vertex back.
  align        (include/viso_hip.h, "TSDF align") Batch.align_tsdf of the first --align-frames (16) resident maps against the table, each
               from its fusing pose moved by 0.2 degrees and 2 cm, min_weight 2, gate 1 voxel: `linearize`, the call with max_iters 1
               (two rounds of one launch each: time per round and per frame and round), and `align`, the call with max_iters 10
               (its rounds: the largest iteration count + 1, from the records).  The yardstick is `render` of the same views in the
               same process (`render_same`): a linearise does eight probes a pixel where a render marches 50..120.
  align_gray   (include/viso_hip.h, "TSDF photometric align") Batch.align_tsdf(photo=True) of the same frames and guesses against the
               gray map, with the resident left images, lambda 1/32: `linearize_gray` (max_iters 1) and `align_gray` (max_iters 10),
               beside `linearize` and `align` in the same process, alternated: 16 more 8-byte loads a run head, one more byte a
               pixel, a second set of 28 products.
  fuse_options (with --carve C, --carve-near M and / or --depth-weights S; include/viso_hip.h, "TSDF fuse options") Batch.fuse_tsdf of
               the same maps into a cleared map of its own with those options (weight_max 255): the extended kernel, in the same
               loop as fuse_tsdf, with its n_updates / n_points and its ratio to fuse_tsdf.  Its table is the first capacity from
               --options-capacity-log2 (default: fuse_tsdf's) on that holds the carved scene; give one that does, since every
               update that finds a table full probes all of its slots.  --fuse-only: only clear, fuse_tsdf and fuse_options are run.
  distance_field  (with --distance-field, which runs only this section; include/viso_hip.h, "TSDF distance field")
               TsdfMap.distance_field over boxes of 256 x 256 x 64 and 512 x 512 x 64 voxels around the camera position of the middle
               frame, min_weight 2, with and without unknown_is_site: the four launches, the copy of sq and state to the host (5
               bytes a cell) and the free.  Where scipy imports, scipy.ndimage.distance_transform_edt of the same site grid on the
               host beside it, as context.
  travel_field  (with --travel-field, which runs only this section; include/viso_hip.h, "TSDF travel field")
               TsdfMap.travel_field over the same two boxes, the goal the middle frame's camera voxel, min_weight 2, at a clearance
               of 0 and of 3 voxels (clearance_sq 0 and 9), with and without unknown_is_site: the distance field's launches, the
               starting costs, the rounds of the relaxation, the copy of cost, sq and state to the host (9 bytes a cell) and the
               free; with each the rounds, n_goals_used and n_reached, and TsdfMap.distance_field of the same box and flag beside
               it in the same loop: the part of the time that the travel field did not add.  Where the camera's own voxel is not
               free in a case (a site, behind the surface, nearer to a site than the clearance), the goal is the free cell nearest
               to it; the result names the goal used.
  retract      (with --retract, which runs only this section; include/viso_hip.h, "TSDF retract") on the map of all resident frames,
               alternated, each call followed outside the clock by what restores the map: Batch.retract_tsdf of one frame (the
               middle one), of 16 frames (from the middle one on) and of all frames, which leaves the map empty; Batch.move_tsdf of
               the 16 frames to poses 2 cm and 0.2 degrees off, and back; Batch.fuse_tsdf of the 16 frames and of all frames into the
               map without them (the yardsticks: a take is the fuse's march); and viso_tsdf_clear followed by Batch.fuse_tsdf of
               all frames, what a 16-frame move replaces.  The result says whether the map at the end is the map at the start.
n_updates / n_points from viso_tsdf_stats is the number of voxels a pixel's band touches.  --kernel-only runs clear + fuse_tsdf
--reps times, the extractions and the render once and the two align calls --reps times: the run to put under `rocprofv3 --kernel-trace --stats` for the kernels' own times.  The
count the result is held against (not a measurement) is printed with it."""
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
    """A count, not a measurement: every map read once (2 B a pixel) over 8 TB/s.  A floor for the pass: neither the table's atomics
    nor the five double divisions a sample are in it."""
    b = float(rows) * cols * nf * 2
    return b, b / 8e12 * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--capacity-log2", type=int, default=26)
    ap.add_argument("--render-views", type=int, default=16)
    ap.add_argument("--align-frames", type=int, default=16)
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--carve", type=int, default=0)
    ap.add_argument("--carve-near", type=float, default=0.0)
    ap.add_argument("--depth-weights", type=int, default=None, metavar="S")
    ap.add_argument("--options-capacity-log2", type=int, default=None)
    ap.add_argument("--fuse-only", action="store_true")
    ap.add_argument("--distance-field", action="store_true")
    ap.add_argument("--travel-field", action="store_true")
    ap.add_argument("--retract", action="store_true")
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
    for log2 in sorted({a.capacity_log2, 27, 28}):
        if log2 < a.capacity_log2:
            continue
        tsdf = libviso_amd.TsdfMap(ctx, capacity_log2=log2)
        try:
            b.fuse_tsdf(tsdf, poses)
            break
        except libviso_amd.VisoError as e:
            tsdf.close()
            if "-4" not in str(e) or log2 == 28:
                raise

    # --carve / --depth-weights: a second map with those fuse options, of the first capacity that holds what it carves
    options = dict(carve_voxels=a.carve, carve_near=a.carve_near, weight_shift=a.depth_weights)
    omap, olog2 = None, log2
    if a.carve or a.depth_weights is not None:
        for olog2 in range(log2 if a.options_capacity_log2 is None else a.options_capacity_log2, 29):
            omap = libviso_amd.TsdfMap(ctx, capacity_log2=olog2, **options)
            try:
                b.fuse_tsdf(omap, poses)
                break
            except libviso_amd.VisoError as e:
                omap.close()
                if "-4" not in str(e) or olog2 == 28:
                    raise

    def fuse_legs(reps):
        """clear, fuse_tsdf and fuse_options alone, alternated."""
        legs = {"clear": [], "fuse_tsdf": []}
        if omap is not None:
            legs["fuse_options"] = []
        for _ in range(reps):
            legs["clear"].append(clock(tsdf.clear))
            legs["fuse_tsdf"].append(clock(lambda: b.fuse_tsdf(tsdf, poses)))
            if omap is not None:
                omap.clear()
                legs["fuse_options"].append(clock(lambda: b.fuse_tsdf(omap, poses)))
        return legs

    def options_result(ms_options, ms_plain):
        so = omap.stats()
        return {"options": options, "capacity_log2": olog2, "stats": so, "updates_per_point": so["n_updates"] / max(1, so["n_points"]),
                "ratio_to_plain": ms_options / ms_plain}

    if a.fuse_only:
        fuse_legs(2)   # warm-up
        legs = fuse_legs(a.reps)
        st = tsdf.stats()
        res = {"frames": nf, "shape": [int(rows), int(cols)], "capacity_log2": log2, "reps": a.reps,
               "ms_median": {k: float(np.median(v)) for k, v in legs.items()}, "ms_min": {k: float(np.min(v)) for k, v in legs.items()},
               "ms_max": {k: float(np.max(v)) for k, v in legs.items()}, "stats": st, "updates_per_point": st["n_updates"] / max(1, st["n_points"])}
        if omap is not None:
            res["fuse_options"] = options_result(res["ms_median"]["fuse_options"], res["ms_median"]["fuse_tsdf"])
            omap.close()
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        tsdf.close(); b.close(); ctx.close()
        return

    if a.retract:
        n16 = min(16, nf)
        t0 = min(nf // 2, nf - n16)
        off = hostmath.tr2mat([0.002, -0.002, 0.002, 0.012, -0.01, 0.012])
        there = np.array([poses[t] @ off for t in range(t0, t0 + n16)])
        start = tsdf.entries().tobytes()
        legs = {k: [] for k in ("retract_1", "fuse_1", "retract_16", "fuse_16", "retract_all", "fuse_tsdf", "move_16", "move_16_back", "clear_and_fuse_all")}
        reports = {}
        for rep_ in range(a.reps + 1):   # alternating; the first round is the warm-up
            ms = {}
            ms["retract_1"] = clock(lambda: reports.__setitem__("retract_1", b.retract_tsdf(tsdf, poses[t0:t0 + 1], t0=t0, t1=t0 + 1)))
            ms["fuse_1"] = clock(lambda: b.fuse_tsdf(tsdf, poses[t0:t0 + 1], t0=t0, t1=t0 + 1))
            ms["retract_16"] = clock(lambda: reports.__setitem__("retract_16", b.retract_tsdf(tsdf, poses[t0:t0 + n16], t0=t0, t1=t0 + n16)))
            ms["fuse_16"] = clock(lambda: b.fuse_tsdf(tsdf, poses[t0:t0 + n16], t0=t0, t1=t0 + n16))
            ms["retract_all"] = clock(lambda: reports.__setitem__("retract_all", b.retract_tsdf(tsdf, poses)))
            ms["fuse_tsdf"] = clock(lambda: b.fuse_tsdf(tsdf, poses))
            ms["move_16"] = clock(lambda: reports.__setitem__("move_16", b.move_tsdf(tsdf, poses[t0:t0 + n16], there, t0=t0, t1=t0 + n16)))
            ms["move_16_back"] = clock(lambda: b.move_tsdf(tsdf, there, poses[t0:t0 + n16], t0=t0, t1=t0 + n16))
            ms["clear_and_fuse_all"] = clock(lambda: (tsdf.clear(), b.fuse_tsdf(tsdf, poses)))
            if rep_:
                for k, v in ms.items():
                    legs[k].append(v)
        st = tsdf.stats()
        med = {k: float(np.median(v)) for k, v in legs.items()}
        res = {"frames": nf, "shape": [int(rows), int(cols)], "capacity_log2": log2, "reps": a.reps, "frames_16": [int(t0), int(t0 + n16)],
               "ms_median": med, "ms_min": {k: float(np.min(v)) for k, v in legs.items()}, "ms_max": {k: float(np.max(v)) for k, v in legs.items()},
               "reports": reports, "stats": st, "same_map_at_the_end": bool(tsdf.entries().tobytes() == start),
               "ratio": {"retract_all_to_fuse_tsdf": med["retract_all"] / med["fuse_tsdf"], "retract_16_to_fuse_16": med["retract_16"] / med["fuse_16"],
                         "move_16_to_clear_and_fuse_all": med["move_16"] / med["clear_and_fuse_all"]}}
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        if omap is not None:
            omap.close()
        tsdf.close(); b.close(); ctx.close()
        return

    if a.travel_field:
        mid = np.floor(poses[nf // 2][:3, 3] / tsdf.voxel).astype(np.int64)
        res = {"frames": nf, "capacity_log2": log2, "reps": a.reps, "min_weight": 2, "goal": [int(v) for v in mid], "boxes": {}}
        for shape in ((256, 256, 64), (512, 512, 64)):
            half = np.array(shape) // 2
            box = (mid - half, mid - half + np.array(shape))
            r = {"box": [[int(v) for v in box[0]], [int(v) for v in box[1]]], "cases": {}}
            for unknown in (False, True):
                for clearance_sq in (0, 9):
                    goal = mid
                    call = lambda: tsdf.travel_field(box, [goal], clearance_sq=clearance_sq, min_weight=2, unknown_is_site=unknown)  # noqa: E731
                    first = call()
                    if not first.n_goals_used:   # the camera's own voxel is not free (a site, behind the surface, too near): the free cell nearest to it
                        sq, st = first.field.sq, first.field.state
                        site = ((st & 4) != 0) | ((st & 3) == 0 if unknown else False)
                        cells = np.argwhere(((st & 3) != 2) & ~site & (sq >= clearance_sq))
                        if len(cells):
                            goal = cells[((cells - (mid - box[0])) ** 2).sum(axis=1).argmin()] + box[0]
                    legs = {"travel_field": [], "distance_field": []}
                    for rep_ in range(a.reps + 1):   # alternating; the first round is the warm-up
                        ms = clock(call), clock(lambda: tsdf.distance_field(box, min_weight=2, unknown_is_site=unknown))
                        if rep_:
                            legs["travel_field"].append(ms[0])
                            legs["distance_field"].append(ms[1])
                    f = call()
                    r["cases"][f"{'unknown_is_site' if unknown else 'surface'}, clearance_sq {clearance_sq}"] = {
                        "goal": [int(v) for v in goal], "rounds": f.rounds, "n_goals_used": f.n_goals_used, "n_reached": f.n_reached,
                        "cost_max": int(f.cost[f.cost != 0xffffffff].max()) if f.n_reached else None,
                        "ms_median": {k: float(np.median(v)) for k, v in legs.items()}, "ms_min": {k: float(np.min(v)) for k, v in legs.items()},
                        "ms_max": {k: float(np.max(v)) for k, v in legs.items()}}
            res["boxes"]["x".join(str(v) for v in shape)] = r
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        if omap is not None:
            omap.close()
        tsdf.close(); b.close(); ctx.close()
        return

    if a.distance_field:
        try:
            from scipy import ndimage
        except ImportError:
            ndimage = None
        mid = np.floor(poses[nf // 2][:3, 3] / tsdf.voxel).astype(np.int64)
        res = {"frames": nf, "capacity_log2": log2, "reps": a.reps, "min_weight": 2, "voxels": int(len(tsdf.entries(2))), "boxes": {}}
        for shape in ((256, 256, 64), (512, 512, 64)):
            half = np.array(shape) // 2
            box = (mid - half, mid - half + np.array(shape))
            legs = {"surface": [], "unknown_is_site": []}
            for rep_ in range(a.reps + 1):   # alternating; the first round is the warm-up
                for name in legs:
                    ms = clock(lambda: tsdf.distance_field(box, min_weight=2, unknown_is_site=name == "unknown_is_site"))
                    if rep_:
                        legs[name].append(ms)
            f = tsdf.distance_field(box, min_weight=2)
            fu = tsdf.distance_field(box, min_weight=2, unknown_is_site=True)
            r = {"box": [[int(v) for v in box[0]], [int(v) for v in box[1]]], "n_sites": f.n_sites, "n_sites_unknown_is_site": fu.n_sites,
                 "unknown_share": float((f.state == 0).mean()), "sq_max": int(f.sq[f.sq != 0xffffffff].max()) if f.n_sites else None,
                 "ms_median": {k: float(np.median(v)) for k, v in legs.items()}, "ms_min": {k: float(np.min(v)) for k, v in legs.items()},
                 "ms_max": {k: float(np.max(v)) for k, v in legs.items()}}
            if ndimage is not None:
                site = (f.state & 4) != 0
                host = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    edt = ndimage.distance_transform_edt(~site)
                    host.append((time.perf_counter() - t0) * 1e3)
                r["scipy_edt_ms_median"] = float(np.median(host))
                r["scipy_agrees"] = bool(f.n_sites == 0 or np.array_equal(np.rint(edt * edt).astype(np.uint32), f.sq))
            res["boxes"]["x".join(str(v) for v in shape)] = r
        print(json.dumps(res))
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
        if omap is not None:
            omap.close()
        tsdf.close(); b.close(); ctx.close()
        return

    views = poses[np.linspace(0, nf - 1, max(1, min(a.render_views, nf))).astype(int)]

    def render():
        return tsdf.render(seq["param"], (rows, cols), views, max_depth=40.0, min_weight=2)

    def marched(d16):
        """Samples marched for the views d16, counted from the result (see above)."""
        h, N = tsdf.voxel * 0.5, int(np.floor(40.0 / (tsdf.voxel * 0.5)))
        valid = d16 != -16
        zs = seq["param"].f * seq["param"].base / (np.where(valid, d16, 16).astype(np.float64) / 16.0)
        return int(np.where(valid, np.minimum(np.ceil(zs / h), N), N).sum()), float(valid.mean())

    has_align = hasattr(libviso_amd.load(), "viso_tsdf_linearize")   # (absent from older builds of the library: VISO_HIP_SO A/B runs)
    na = max(1, min(a.align_frames, nf))
    guesses = np.array([poses[t] @ hostmath.tr2mat([0.002, -0.002, 0.002, 0.012, -0.01, 0.012]) for t in range(na)])

    def align(max_iters):
        return b.align_tsdf(tsdf, guesses, t0=0, t1=na, max_iters=max_iters)

    has_align_gray = hasattr(libviso_amd.load(), "viso_tsdf_linearize_gray")   # (likewise)

    def align_gray(max_iters):
        return b.align_tsdf(gmap, guesses, t0=0, t1=na, photo=True, max_iters=max_iters)

    def render_same():
        return tsdf.render(seq["param"], (rows, cols), poses[:na], max_depth=40.0, min_weight=2)

    if a.kernel_only:
        ms = []
        for _ in range(a.reps):
            tsdf.clear()
            ms.append(clock(lambda: b.fuse_tsdf(tsdf, poses)))
        res = {"frames": nf, "fuse_tsdf_ms": ms, "voxels": int(len(tsdf.entries())), "crossings": int(len(tsdf.surface())),
               "triangles": int(len(tsdf.mesh()[1])), "render_views": int(len(views)), "render_valid": marched(render())[1]}
        if has_align:
            res["align_ms"] = [[clock(lambda: align(1)), clock(lambda: align(10))] for _ in range(a.reps)]
        print(json.dumps(res))
        tsdf.close(); b.close(); ctx.close()
        return

    vmap = libviso_amd.VoxelMap(ctx, capacity_log2=26)
    has_gray = hasattr(libviso_amd.load(), "viso_tsdf_create_gray")   # (absent from older builds of the library: VISO_HIP_SO A/B runs)
    if has_gray:
        gmap = libviso_amd.TsdfMap(ctx, gray=True, capacity_log2=log2)
        b.fuse_tsdf(gmap, poses)
        gverts = gmap.mesh()[0]

    def render_gray():
        return gmap.render(seq["param"], (rows, cols), views, max_depth=40.0, min_weight=2, gray=True)

    has_normals = hasattr(libviso_amd.load(), "viso_tsdf_render_normals")   # (likewise)

    def render_normals():
        return tsdf.normals.render(seq["param"], (rows, cols), views, max_depth=40.0, min_weight=2)

    for _ in range(2):   # warm-up
        tsdf.clear(); b.fuse_tsdf(tsdf, poses); tsdf.entries(); tsdf.surface(); tsdf.mesh(); render()
        if has_normals:
            render_normals(); tsdf.normals.mesh()
        vmap.clear(); b.fuse_disparities(vmap, poses)
        if has_gray:
            gmap.clear(); b.fuse_tsdf(gmap, poses); gmap.vertex_gray(gverts); render_gray()
        if has_align:
            align(1); align(10); render_same()
        if has_align_gray:
            align_gray(1); align_gray(10)
    legs = {k: [] for k in ("fuse_tsdf", "fuse_map", "entries", "surface", "mesh", "render", "clear") + (("fuse_gray", "vertex_gray", "render_gray") if has_gray else ())
            + (("linearize", "align", "render_same") if has_align else ()) + (("linearize_gray", "align_gray") if has_align_gray else ())
            + (("fuse_options",) if omap is not None else ()) + (("render_normals", "mesh_normals") if has_normals else ())}
    for _ in range(a.reps):   # alternating
        legs["clear"].append(clock(tsdf.clear))
        legs["fuse_tsdf"].append(clock(lambda: b.fuse_tsdf(tsdf, poses)))
        if omap is not None:
            omap.clear()
            legs["fuse_options"].append(clock(lambda: b.fuse_tsdf(omap, poses)))
        vmap.clear()
        legs["fuse_map"].append(clock(lambda: b.fuse_disparities(vmap, poses)))
        legs["entries"].append(clock(tsdf.entries))
        legs["surface"].append(clock(tsdf.surface))
        legs["mesh"].append(clock(tsdf.mesh))
        legs["render"].append(clock(render))
        if has_normals:
            legs["mesh_normals"].append(clock(tsdf.normals.mesh))
            legs["render_normals"].append(clock(render_normals))
        if has_gray:
            gmap.clear()
            legs["fuse_gray"].append(clock(lambda: b.fuse_tsdf(gmap, poses)))
            legs["vertex_gray"].append(clock(lambda: gmap.vertex_gray(gverts)))
            legs["render_gray"].append(clock(render_gray))
        if has_align:
            legs["linearize"].append(clock(lambda: align(1)))
            legs["align"].append(clock(lambda: align(10)))
            legs["render_same"].append(clock(render_same))
        if has_align_gray:
            legs["linearize_gray"].append(clock(lambda: align_gray(1)))
            legs["align_gray"].append(clock(lambda: align_gray(10)))
    st, n_vox, n_cross = tsdf.stats(), len(tsdf.entries()), len(tsdf.surface())
    n_vert, n_tri = (len(x) for x in tsdf.mesh())
    res = {"frames": nf, "shape": [int(rows), int(cols)], "params": "voxel 0.2, T 3, min_disp16 16", "capacity_log2": log2, "reps": a.reps,
           "ms_median": {k: float(np.median(v)) for k, v in legs.items()}, "ms_min": {k: float(np.min(v)) for k, v in legs.items()},
           "ms_max": {k: float(np.max(v)) for k, v in legs.items()},
           "stats": st, "voxels": int(n_vox), "crossings": int(n_cross), "vertices": int(n_vert), "triangles": int(n_tri), "updates_per_point": st["n_updates"] / max(1, st["n_points"]),
           "map_stats": vmap.stats()}
    res["count_bytes"], res["count_ms"] = count_ms(nf, rows, cols)
    n_marched, valid = marched(render())
    ms = res["ms_median"]["render"]
    res["render"] = {"views": int(len(views)), "max_depth": 40.0, "min_weight": 2, "valid": valid, "ms_per_view": ms / len(views),
                     "samples_marched": n_marched, "samples_per_s": n_marched / (ms * 1e-3)}
    if has_normals:
        d16, nrm = render_normals()
        nv = tsdf.normals.mesh()[2]
        med = res["ms_median"]
        res["normals"] = {"ms_per_view": med["render_normals"] / len(views), "render_ratio_to_plain": med["render_normals"] / med["render"],
                          "pixels_with_normal_of_valid": float(nrm.any(axis=-1).sum() / max(1, int((d16 != -16).sum()))),
                          "mesh_ratio_to_plain": med["mesh_normals"] / med["mesh"], "vertex_normals_ms": med["mesh_normals"] - med["mesh"],
                          "vertices_with_normal": float(nv.any(axis=1).mean()) if len(nv) else 0.0}
    if has_align:
        r1, r10, med = align(1), align(10), res["ms_median"]
        rounds1, rounds10 = int(r1["iters"].max()) + 1, int(r10["iters"].max()) + 1
        res["align"] = {"frames": na, "min_weight": 2, "gate_voxels": 1.0, "status_max_iters_1": [int(v) for v in r1["status"]],
                        "status": [int(v) for v in r10["status"]], "iters": [int(v) for v in r10["iters"]],
                        "n_used_share": float(r10["n_used"].mean() / (rows * cols)), "rounds_max_iters_1": rounds1, "rounds": rounds10,
                        "ms_per_round_max_iters_1": med["linearize"] / rounds1, "ms_per_frame_and_round": med["linearize"] / rounds1 / na,
                        "ms_per_align_call": med["align"], "ms_per_round": med["align"] / rounds10,
                        "render_same_ms_per_view": med["render_same"] / na}
    if has_align_gray:
        g1, g10, med = align_gray(1), align_gray(10), res["ms_median"]
        rounds1, rounds10 = int(g1["iters"].max()) + 1, int(g10["iters"].max()) + 1
        res["align_gray"] = {"frames": na, "photo_weight": 1.0 / 32.0, "status": [int(v) for v in g10["status"]], "iters": [int(v) for v in g10["iters"]],
                             "n_photo_used_share": float(g10["n_photo_used"].mean() / (rows * cols)), "rounds_max_iters_1": rounds1, "rounds": rounds10,
                             "cost_geo_px": float(g10["cost_geo"].mean()), "cost_photo_gray": float(g10["cost_photo"].mean()),
                             "ms_per_round_max_iters_1": med["linearize_gray"] / rounds1, "ms_per_frame_and_round": med["linearize_gray"] / rounds1 / na,
                             "ms_per_align_call": med["align_gray"], "ms_per_round": med["align_gray"] / rounds10,
                             "ratio_to_plain_per_round": (med["linearize_gray"] / rounds1) / (med["linearize"] / max(1, int(align(1)["iters"].max()) + 1))}
    if omap is not None:
        res["fuse_options"] = options_result(res["ms_median"]["fuse_options"], res["ms_median"]["fuse_tsdf"])
        omap.close()
    if has_gray:
        res["gray"] = {"vertices": int(len(gverts)), "same_geometry": bool(gmap.entries().tobytes() == tsdf.entries().tobytes()),
                       "ratio_to_plain": {g: res["ms_median"][g] / res["ms_median"][p] for g, p in (("fuse_gray", "fuse_tsdf"), ("render_gray", "render"))}}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    tsdf.close(); vmap.close()
    if has_gray:
        gmap.close()
    b.close(); ctx.close()


if __name__ == "__main__":
    main()
