// tsdf.hip — opt-in TSDF map: dense disparity maps and poses fused into a hash table of truncated signed distances on the device,
// and the sign changes between neighbouring voxels read back as surface crossings (NOT in the reference: viso_tsdf_*,
// viso_batch_fuse_tsdf, include/viso_hip.h) or as a triangle mesh by marching tetrahedra.
//
// The table is the voxel map's (voxel_hash.h): keys [slots] u64 (all ones = empty), weight [slots] u32, sum [slots] i64 (added as
// u64, two's complement).  A key is claimed with one 64-bit compare-and-swap; everything added behind it is an integer atomic add,
// so the table after any set of calls depends on neither their order nor on scheduling.  Every probe loop is bounded by the capacity
// and advances strictly; no workgroup waits for another one.  No kernel uses scratch or LDS.
//
//   tsdf_fuse_kernel         one thread per pixel of a group of frames.  The loop over the 4T + 1 samples of a pixel's ray is uniform
//                            across the wave: every lane is at the same j, so neighbouring pixels mostly land in the same voxel.  Per j
//                            the lanes that continue the key of the lane to their left form a run: the run heads from one ballot, the
//                            run's sum of q (biased by T 1024, so unsigned: 64 x 2 x 8 x 1024 < 2^21) from one wave scan (DPP) and
//                            one exchange with the run's last lane.  Only the head lane probes the table and issues the two atomic
//                            adds (weight, sum).  Lanes that skip a sample take part as runs of the empty key.
//   tsdf_crossings_kernel    one thread per slot, three read-only probes for the neighbours at +1 on every axis: the sign changes
//                            between voxels of weight >= min_weight to a dense list, one atomic per wave for the list positions
//                            (out == null: only their number), in the getters' two passes.
//   tsdf_mesh_kernel         one thread per slot, seven read-only probes for the other corners of the voxel's cell: the sign-changing
//                            edges the voxel owns as vertices, and the triangles of the cell's six tetrahedra as references to
//                            them; two lists, one atomic per wave and list; the same two passes.
//   tsdf_render_kernel       one thread per pixel of a group of views, reads only (include/viso_hip.h, "TSDF render").
//                            The march over the samples of a pixel's ray is uniform across the wave, with the runs of the fuse
//                            kernel: only a run's head lane probes the table (voxel_find) and loads weight and sum, the other
//                            lanes of the run take them from it (three ds_bpermute).  Ends when no lane of the wave marches.
// A gray map (include/viso_hip.h, "TSDF intensity") carries a third payload array, gray [slots] u64, the sum of the
// 8-bit intensities of the pixels that updated a voxel.  Its kernels are their plain counterparts with that array carried: the
// fuse and the render share their bodies with them (template <bool GRAY>, the plain instance reads none of the three extra
// arguments).
//   tsdf_gray_fuse_kernel         the fuse kernel's march with the pixel's intensity (one byte a pixel, along the row); the run's
//                                 sum of intensities from a second wave scan (64 x 255 < 2^14), a third atomic add from its head lane.
//   tsdf_gray_sample_kernel       one thread per vertex (k, dir): two read-only probes for the ends of its edge, the intensity
//                                 interpolated with the mesh's t; the vertices without a value counted with one atomic per wave.
//   tsdf_gray_render_kernel       the render march; a run's head lane also loads gray and hands it to its run (two more
//                                 ds_bpermute for the 64-bit value).
// The surface normals (include/viso_hip.h, "TSDF normals") read weight and sum only, of a plain or a gray map:
//   tsdf_normal_sample_kernel     one thread per vertex (k, dir): two read-only probes for the ends of its edge, then the gradients
//                                 of the two voxels over their six neighbours (ten more probes for an axis edge, twelve otherwise),
//                                 interpolated with the mesh's t; the vertices without a normal counted with one atomic per wave.
//   tsdf_normal_render_kernel     the render march unchanged (a third instance of its body); a lane keeps the two voxels of its hit,
//                                 and the twelve probes of the two gradients run behind the march, where the wave is converged.
// A map's fuse options (include/viso_hip.h, "TSDF fuse options") add two instances of the fuse body (template
// <bool GRAY, bool EXT>; without EXT none of the options is read and the two kernels above are what they were):
//   tsdf_carve_fuse_kernel        the fuse kernel's march from 2 C samples earlier, started per wave at the first j at which one of
//   tsdf_gray_carve_fuse_kernel   its lanes has a sample to insert (one wave minimum, wave.h), with the pixel's weight w carried: the
//                                 run's sums of w, w (q + T 1024) and w I from one wave scan each, the run's length only for the
//                                 dropped counter.  Launched only for a map whose options are not the defaults.
// A retract (include/viso_hip.h, "TSDF retract") takes the updates of fused frames out of the table again, four
// more instances of the fuse body (template <.., bool TAKE>; without TAKE the four kernels above are what they were):
//   tsdf_take_kernel              the fuse kernels' march, run for run; a run's head lane finds its slot (voxel_find: no slot is
//   tsdf_gray_take_kernel         claimed, no key written), adds the negated sums -- or, with the runtime flag undo, the sums
//   tsdf_carve_take_kernel        themselves -- and compares the weight its own atomic returns with what it took.  The updates that
//   tsdf_gray_carve_take_kernel   found no voxel and the underflow flag: one atomic per wave and word, only when not zero.
// The check and the mark that follow are voxel_hash.h's, over TsdfPayload; the rebuild and the sweep are the eviction's.
// The frame-to-model alignment that reads this table is in tsdf_align.hip (the table's layout: tsdf_table.h).
// What every table of voxels shares is not here (voxelmap.hip says what): the device side is voxel_hash.h, the host side
// voxel_host.h.  The kernels that list, clear, add entries to and evict slots are voxel_hash.h's templates, instantiated here over
// TsdfPayload<false> (a plain map) and TsdfPayload<true> (a gray map).  This file keeps the table's payload, the other kernels and
// the fuse's insert, the parameter and entry checks, the orders of the items and the whole mesh extraction, whose two lists do not
// fit the shared two passes.
#include "common.h"
#include "wave.h"
#include "tsdf_table.h"

#include <cmath>
#include <type_traits>
#include <vector>

// a gray map's table (include/viso_hip.h, "TSDF intensity"): the same with the sums of the updates' 8-bit intensities
struct TsdfGrayTable {
    TsdfTable t;
    unsigned long long* gray;                    // [slots]
};

// `updates` updates of the weights' sum `weight` and the sum of w q `sum` into the voxel `key`; gray_at set (a gray map): and
// their sum of w I `gray`.  The dropped counter counts updates, not weights.
__device__ __forceinline__ void tsdf_insert(const TsdfTable& t, unsigned long long key, uint32_t updates, uint32_t weight, long long sum,
                                            bool* claimed, unsigned long long* gray_at = nullptr, unsigned long long gray = 0) {
    uint32_t slot;
    if (voxel_probe(t.head.keys, t.head.mask, key, &slot, claimed)) {
        atomicAdd(t.weight + slot, weight);
        atomicAdd(t.sum + slot, (unsigned long long)sum);
        if (gray_at) atomicAdd(gray_at + slot, gray);
    } else {
        atomicAdd(t.head.words + VOXEL_W_DROPPED, (unsigned long long)updates);
    }
}

// The take's twin of tsdf_insert (include/viso_hip.h, "TSDF retract"): the same sums out of the voxel `key`, in the table's own
// modular arithmetic, through a read-only probe: no slot is claimed and no key written.  A voxel that is not in the table: its
// updates to *missing; a weight that the take brings below zero (the value its own atomic returns is smaller than what it takes):
// *under set.  undo: the sums go back in, and neither is noted.
__device__ __forceinline__ void tsdf_take(const TsdfTable& t, unsigned long long key, uint32_t updates, uint32_t weight, long long sum, bool undo,
                                          uint32_t* missing, bool* under, unsigned long long* gray_at = nullptr, unsigned long long gray = 0) {
    uint32_t slot;
    if (voxel_find(t.head.keys, t.head.mask, key, &slot)) {
        const uint32_t old = atomicAdd(t.weight + slot, undo ? weight : 0u - weight);
        atomicAdd(t.sum + slot, undo ? (unsigned long long)sum : 0ull - (unsigned long long)sum);
        if (gray_at) atomicAdd(gray_at + slot, undo ? gray : 0ull - gray);
        if (!undo && old < weight) *under = true;
    } else if (!undo) {
        *missing += updates;
    }
}

struct TsdfFuseArgs {
    VoxelFuseArgs v;
    int trunc;
    double s, h;
    TsdfTable t;
};

struct TsdfGrayFuseArgs {
    TsdfFuseArgs a;
    const uint8_t* image; size_t ifs;   // frame f's left image at image + f * ifs, pixel for pixel the map's
    unsigned long long* gray;
};

// a map's fuse options as the extended kernels take them (include/viso_hip.h, "TSDF fuse options"); checked on the host
struct TsdfFuseOpts {
    int carve;                          // C
    int weight_shift;                   // < 0: every update weighs 1
    uint32_t weight_max; int _pad;
    double carve_near;
};

// the sum of v over this lane's run, in the run's head lane (len: voxel_runs'); every lane of the wave calls
__device__ __forceinline__ uint32_t tsdf_run_sum(uint32_t v, int lane, uint32_t len) {
    const uint32_t s = viso_wave_scan(v);                                         // inclusive prefix
    return (uint32_t)__shfl((int)s, lane + (int)len - 1) - s + v;
}

// The body of the fuse kernels.  GRAY: the pixel's intensity (image, ifs) is carried along, and a run's head lane adds the run's
// sum of intensities to gray[slot] as well; without it, none of the three is read.  EXT: the rules of "TSDF fuse options": the
// loop starts 2 o.carve samples earlier, and a pixel's updates carry its weight w; without it, o is not read.  TAKE: the march of a
// retract ("TSDF retract"): a run's head lane hands the run's sums to tsdf_take and not to tsdf_insert, the wave's counters fall by
// what the fuse adds, and what the wave could not place or took below zero goes to VOXEL_W_MISSING and VOXEL_W_UNDERFLOW, one
// atomic per wave and word that is not zero; undo: the same march puts everything back.  Without TAKE, undo is not read.
template <bool GRAY, bool EXT, bool TAKE = false>
__device__ __forceinline__ void tsdf_fuse_body(const TsdfFuseArgs& a, const TsdfFuseOpts& o, const uint8_t* image, size_t ifs,
                                               unsigned long long* gray, bool undo = false) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, fr = blockIdx.y;
    double X = 0.0, Y = 0.0, Z = 1.0;
    const bool point = voxel_point(a.v, i, fr, &X, &Y, &Z);
    const unsigned long long pm = __ballot(point);
    if (!pm) return;   // the whole wave
    uint32_t pix = 0;                               // one byte a pixel, the lanes of a wave consecutive bytes of a row
    if (GRAY && point) pix = image[(size_t)fr * ifs + i];
    uint32_t w = 1;                                 // what each of the pixel's updates weighs
    int j_first = -2 * a.trunc;
    if constexpr (EXT) {
        if (point && o.weight_shift >= 0) {
            const uint32_t d16 = (uint32_t)a.v.disp[(size_t)fr * a.v.mfs + i];    // 1 .. 32767: its square fits
            w = min(max((d16 * d16) >> o.weight_shift, 1u), o.weight_max);
        }
        // The wave starts at the smallest j at which one of its lanes has a sample to insert (zj > 0 and zj >= carve_near): zj does
        // not fall as j grows, so a lane's earlier samples insert nothing and only reset a `prev` that is empty already.  The
        // lane's own first such j: an estimate one sample early from the division, then moved down while the sample before it
        // still is one, with the very expression of the loop below, so that no rounding of the estimate can skip a sample.
        const int j0 = -2 * (a.trunc + o.carve);
        int jl = 2 * a.trunc + 1;
        if (point) {
            jl = (int)fmin(fmax(floor((o.carve_near - Z) / a.h) - 1.0, (double)j0), (double)(-2 * a.trunc));
            while (jl > j0) {
                const double zb = Z + (double)(jl - 1) * a.h;
                if (!(zb > 0.0 && zb >= o.carve_near)) break;
                --jl;
            }
        }
        j_first = j0 + (int)wave_min_u32((uint32_t)(jl - j0));
    }
    // Without a pose the identity: ((1 a + 0 b) + 0 c) + 0 = a and (0 a + 0 b) + 1 (c - 0) = c for finite a, b, c, up to the sign
    // of a zero, which neither floor(. / s) nor Z - zc keeps.
    double T0 = 1.0, T1 = 0.0, T2 = 0.0, T3 = 0.0, T4 = 0.0, T5 = 1.0, T6 = 0.0, T7 = 0.0, T8 = 0.0, T9 = 0.0, T10 = 1.0, T11 = 0.0;
    if (a.v.poses) {
        const double* T = a.v.poses + (size_t)fr * 12;
        T0 = T[0]; T1 = T[1]; T2 = T[2]; T3 = T[3]; T4 = T[4]; T5 = T[5]; T6 = T[6]; T7 = T[7]; T8 = T[8]; T9 = T[9]; T10 = T[10]; T11 = T[11];
    }
    const int lim = a.trunc * 1024;
    const double dlim = (double)lim;
    unsigned long long prev = MAP_EMPTY;            // the voxel of the pixel's previous inserted sample
    unsigned long long n_upd = 0, n_oor = 0, n_occ = 0;
    uint32_t n_miss = 0;                            // TAKE: the updates of this lane's runs that found no voxel (at most 64 a sample)
    bool under = false;                             //       one of this lane's runs took a weight below zero
    // a run's sums from its head lane into the table, or with TAKE out of it
    auto put = [&](unsigned long long key, uint32_t updates, uint32_t weight, long long sum, bool* claimed, unsigned long long* gray_at,
                   unsigned long long run_gray) {
        if constexpr (TAKE) tsdf_take(a.t, key, updates, weight, sum, undo, &n_miss, &under, gray_at, run_gray);
        else tsdf_insert(a.t, key, updates, weight, sum, claimed, gray_at, run_gray);
    };
    for (int j = j_first; j <= 2 * a.trunc; ++j) {   // the same j in every lane
        unsigned long long key = MAP_EMPTY;
        uint32_t qb = 0;                            // q + T 1024
        bool oor = false;
        if (point) {
            const double zj = Z + (double)j * a.h;
            bool on = zj > 0.0;
            if constexpr (EXT) on = on && !(j < -2 * a.trunc && zj < o.carve_near);   // a free-space sample nearer than carve_near
            if (on) {
                const double r = zj / Z;
                const double c0 = X * r, c1 = Y * r;
                const double gx = floor((((T0 * c0 + T1 * c1) + T2 * zj) + T3) / a.s);
                const double gy = floor((((T4 * c0 + T5 * c1) + T6 * zj) + T7) / a.s);
                const double gz = floor((((T8 * c0 + T9 * c1) + T10 * zj) + T11) / a.s);
                if (fabs(gx) < MAP_RANGE && fabs(gy) < MAP_RANGE && fabs(gz) < MAP_RANGE) {   // false for a NaN
                    const int kx = (int)gx >> 10, ky = (int)gy >> 10, kz = (int)gz >> 10;
                    const unsigned long long k = voxel_key(kx, ky, kz);
                    if (k != prev) {
                        const double C0 = (double)(kx * 1024 + 512) * a.s, C1 = (double)(ky * 1024 + 512) * a.s, C2 = (double)(kz * 1024 + 512) * a.s;
                        const double zc = (T2 * (C0 - T3) + T6 * (C1 - T7)) + T10 * (C2 - T11);
                        const double fq = floor((Z - zc) / a.s);
                        if (fq >= -dlim) {          // false for a NaN
                            key = k;
                            qb = (uint32_t)((fq > dlim ? lim : (int)fq) + lim);
                        }
                    }
                    prev = k;
                } else {
                    oor = true;
                    prev = MAP_EMPTY;
                }
            } else {
                prev = MAP_EMPTY;
            }
        }
        n_oor += __popcll(__ballot(oor));
        const unsigned long long um = __ballot(key != MAP_EMPTY);
        if (!um) continue;   // the whole wave
        n_upd += __popcll(um);
        // the runs of equal keys along the wave (lanes without an update: runs of the empty key, which insert nothing)
        bool head;
        uint32_t len;
        voxel_runs(key, lane, &head, &len);
        bool claimed = false;
        if constexpr (EXT) {
            // The run's sums of w, of w (q + T 1024) and, on a gray map, of w I, each by a scan of the plain kernel's shape: at most
            // 64 x 255 < 2^14, 64 x 255 x 16384 < 2^28 and 64 x 255 x 255 < 2^22, so 32 bits hold them.  The lanes without an update
            // are runs of the empty key, which insert nothing: what they add to the scans cancels in a run's difference.
            const uint32_t rw = tsdf_run_sum(w, lane, len);
            const uint32_t rq = tsdf_run_sum(w * qb, lane, len);
            const uint32_t rg = GRAY ? tsdf_run_sum(w * pix, lane, len) : 0u;
            if (head && key != MAP_EMPTY)
                put(key, len, rw, (long long)rq - (long long)rw * lim, &claimed, GRAY ? gray : nullptr, rg);
        } else {
            const uint32_t rq = tsdf_run_sum(qb, lane, len);                      // the run's sum, in its head lane
            if (GRAY) {
                // the run's sum of intensities by a second scan of the same shape (64 x 255 < 2^14)
                const uint32_t rg = tsdf_run_sum(key != MAP_EMPTY ? pix : 0u, lane, len);
                if (head && key != MAP_EMPTY) put(key, len, len, (long long)rq - (long long)len * lim, &claimed, gray, rg);
            } else {
                if (head && key != MAP_EMPTY) put(key, len, len, (long long)rq - (long long)len * lim, &claimed, nullptr, 0);
            }
        }
        n_occ += __popcll(__ballot(claimed));
    }
    if constexpr (TAKE) {
        // the counters fall (undo: rise again) by what the fuse adds to them, modulo 2^64 in a set: their sum over the sets is exact
        const unsigned long long sg = undo ? 1ull : ~0ull;
        voxel_count_wave(a.t.head, blockIdx.x + blockIdx.y, lane, sg * (unsigned long long)__popcll(pm), sg * n_upd, sg * n_oor, 0);
        const uint32_t missing = viso_wave_scan(n_miss);   // lane 63: the wave's (at most 64 a sample of at most 2 (8 + 1024) + 1: 32 bits hold it)
        const unsigned long long um = __ballot(under);
        if (lane == 63 && missing) atomicAdd(a.t.head.words + VOXEL_W_MISSING, (unsigned long long)missing);
        if (lane == 0 && um) atomicAdd(a.t.head.words + VOXEL_W_UNDERFLOW, (unsigned long long)__popcll(um));
    } else {
        voxel_count_wave(a.t.head, blockIdx.x + blockIdx.y, lane, __popcll(pm), n_upd, n_oor, n_occ);
    }
}

__global__ __launch_bounds__(256) void tsdf_fuse_kernel(TsdfFuseArgs a) { tsdf_fuse_body<false, false>(a, TsdfFuseOpts{}, nullptr, 0, nullptr); }
__global__ __launch_bounds__(256) void tsdf_gray_fuse_kernel(TsdfGrayFuseArgs g) {
    tsdf_fuse_body<true, false>(g.a, TsdfFuseOpts{}, g.image, g.ifs, g.gray);
}
// the same two with a map's fuse options (launched only when one of them is on)
__global__ __launch_bounds__(256) void tsdf_carve_fuse_kernel(TsdfFuseArgs a, TsdfFuseOpts o) {
    tsdf_fuse_body<false, true>(a, o, nullptr, 0, nullptr);
}
__global__ __launch_bounds__(256) void tsdf_gray_carve_fuse_kernel(TsdfGrayFuseArgs g, TsdfFuseOpts o) {
    tsdf_fuse_body<true, true>(g.a, o, g.image, g.ifs, g.gray);
}
// The four take kernels of a retract: the same four marches with TAKE; undo: a runtime sign, one kernel for both directions.
__global__ __launch_bounds__(256) void tsdf_take_kernel(TsdfFuseArgs a, bool undo) {
    tsdf_fuse_body<false, false, true>(a, TsdfFuseOpts{}, nullptr, 0, nullptr, undo);
}
__global__ __launch_bounds__(256) void tsdf_gray_take_kernel(TsdfGrayFuseArgs g, bool undo) {
    tsdf_fuse_body<true, false, true>(g.a, TsdfFuseOpts{}, g.image, g.ifs, g.gray, undo);
}
__global__ __launch_bounds__(256) void tsdf_carve_take_kernel(TsdfFuseArgs a, TsdfFuseOpts o, bool undo) {
    tsdf_fuse_body<false, true, true>(a, o, nullptr, 0, nullptr, undo);
}
__global__ __launch_bounds__(256) void tsdf_gray_carve_take_kernel(TsdfGrayFuseArgs g, TsdfFuseOpts o, bool undo) {
    tsdf_fuse_body<true, true, true>(g.a, o, g.image, g.ifs, g.gray, undo);
}

// The intensity of the point on the edge between the voxels a and b (include/viso_hip.h, "TSDF intensity"): t is the mesh's and the
// render's, the means of the intensities are interpolated with it.  wa, wb >= 1 and the sums differ in sign.
__device__ __forceinline__ uint8_t tsdf_edge_gray(uint32_t wa, long long sa, unsigned long long ga, uint32_t wb, long long sb, unsigned long long gb) {
    const double da = (double)sa / (double)wa, db = (double)sb / (double)wb;
    const double t = da / (da - db);
    const double ia = (double)ga / (double)wa, ib = (double)gb / (double)wb;
    const double v = ia + (ib - ia) * t;
    return (uint8_t)fmin(255.0, floor(v + 0.5));
}

// One thread per vertex (k, dir), checked on the host: two read-only probes for the ends of its edge.  An end that is not in the
// table, or ends of one sign: 0, and the vertex counts in VOXEL_W_OUT, one atomic per wave.
__global__ __launch_bounds__(256) void tsdf_gray_sample_kernel(TsdfGrayTable g, const viso_tsdf_mesh_vertex* verts, unsigned long long n, uint8_t* out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    bool missing = false;
    if (i < n) {
        const viso_tsdf_mesh_vertex v = verts[i];
        const unsigned long long ka = voxel_key(v.k[0], v.k[1], v.k[2]);
        uint32_t a, b;
        uint8_t val = 0;
        missing = true;
        if (voxel_find(g.t.head.keys, g.t.head.mask, ka, &a) && voxel_find(g.t.head.keys, g.t.head.mask, voxel_neighbour(ka, (uint32_t)v.dir), &b)) {
            const uint32_t wa = g.t.weight[a], wb = g.t.weight[b];
            const long long sa = (long long)g.t.sum[a], sb = (long long)g.t.sum[b];
            if (wa && wb && (sa < 0) != (sb < 0)) {
                val = tsdf_edge_gray(wa, sa, g.gray[a], wb, sb, g.gray[b]);
                missing = false;
            }
        }
        out[i] = val;
    }
    const unsigned long long m = __ballot(missing);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(g.t.head.words + VOXEL_W_OUT, (unsigned long long)__popcll(m));
}

// ---- surface normals (include/viso_hip.h, "TSDF normals") ---------------------------------------------------------
// d = sum / weight of the voxel `key` where it is usable (in the table with weight >= min_weight >= 1): one read-only probe
__device__ __forceinline__ bool tsdf_usable(const TsdfTable& t, unsigned long long key, uint32_t min_weight, double* d) {
    uint32_t slot;
    if (!voxel_find(t.head.keys, t.head.mask, key, &slot)) return false;
    const uint32_t w = t.weight[slot];
    if (w < min_weight) return false;
    *d = (double)(long long)t.sum[slot] / (double)w;
    return true;
}

// G along AX of the usable voxel `key` of distance d: central where both neighbours are usable, one-sided where one is; false:
// neither is.  known 1 / 2: the caller holds the upper / the lower neighbour, usable, of distance dk, and it is not probed again.
template <int AX>
__device__ __forceinline__ bool tsdf_axis_gradient(const TsdfTable& t, unsigned long long key, uint32_t min_weight, double d, int known, double dk,
                                                   double* g) {
    unsigned long long kp, km;
    double dp = dk, dm = dk;
    const bool up = known == 1 || (voxel_step_up(key, AX, &kp) && tsdf_usable(t, kp, min_weight, &dp));
    const bool down = known == 2 || (voxel_step_down(key, AX, &km) && tsdf_usable(t, km, min_weight, &dm));
    if (up && down) *g = (dp - dm) * 0.5;
    else if (up) *g = dp - d;
    else if (down) *g = d - dm;
    else return false;
    return true;
}

// The gradient of the usable voxel `key` of distance d over its six neighbours: six read-only probes, the three axes unrolled, G in
// named scalars.  known_ax in 0..2: one neighbour on that axis is the caller's (known_up: the upper one), of distance dk; -1: none.
// false: an axis without a usable neighbour, the voxel has no gradient.
__device__ __forceinline__ bool tsdf_voxel_gradient(const TsdfTable& t, unsigned long long key, uint32_t min_weight, double d, int known_ax,
                                                    bool known_up, double dk, double* G0, double* G1, double* G2) {
    const int kn = known_up ? 1 : 2;
    return tsdf_axis_gradient<0>(t, key, min_weight, d, known_ax == 0 ? kn : 0, dk, G0) &&
           tsdf_axis_gradient<1>(t, key, min_weight, d, known_ax == 1 ? kn : 0, dk, G1) &&
           tsdf_axis_gradient<2>(t, key, min_weight, d, known_ax == 2 ? kn : 0, dk, G2);
}

// The unit normal in the world frame of the point on the edge between the usable voxels a and b, whose sums differ in sign: the two
// gradients interpolated with the mesh's and the render's t.  axis in 0..2: b is a's upper neighbour on that axis; -1: any two
// voxels.  false: missing (an end without a gradient, or a length that is not positive and finite).
__device__ __forceinline__ bool tsdf_edge_normal(const TsdfTable& t, uint32_t min_weight, unsigned long long ka, uint32_t wa, long long sa,
                                                 unsigned long long kb, uint32_t wb, long long sb, int axis, double* n0, double* n1, double* n2) {
    const double da = (double)sa / (double)wa, db = (double)sb / (double)wb;
    const double tt = da / (da - db);
    double a0, a1, a2, b0, b1, b2;
    if (!tsdf_voxel_gradient(t, ka, min_weight, da, axis, true, db, &a0, &a1, &a2)) return false;
    if (!tsdf_voxel_gradient(t, kb, min_weight, db, axis, false, da, &b0, &b1, &b2)) return false;
    const double g0 = a0 + (b0 - a0) * tt, g1 = a1 + (b1 - a1) * tt, g2 = a2 + (b2 - a2) * tt;
    const double L = sqrt((g0 * g0 + g1 * g1) + g2 * g2);
    if (!(L > 0.0) || !isfinite(L)) return false;
    *n0 = g0 / L; *n1 = g1 / L; *n2 = g2 / L;
    return true;
}

// One thread per vertex (k, dir), checked on the host: two read-only probes for the ends of its edge, then the two gradients (an
// axis edge: each end is the other's neighbour, ten probes; otherwise twelve).  A missing normal: (0, 0, 0), and the vertex counts
// in VOXEL_W_OUT, one atomic per wave.
__global__ __launch_bounds__(256) void tsdf_normal_sample_kernel(TsdfTable t, uint32_t min_weight, const viso_tsdf_mesh_vertex* verts,
                                                                 unsigned long long n, float* out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    bool missing = false;
    if (i < n) {
        const viso_tsdf_mesh_vertex v = verts[i];
        const unsigned long long ka = voxel_key(v.k[0], v.k[1], v.k[2]), kb = voxel_neighbour(ka, (uint32_t)v.dir);
        uint32_t a, b;
        float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
        missing = true;
        if (voxel_find(t.head.keys, t.head.mask, ka, &a) && voxel_find(t.head.keys, t.head.mask, kb, &b)) {
            const uint32_t wa = t.weight[a], wb = t.weight[b];
            const long long sa = (long long)t.sum[a], sb = (long long)t.sum[b];
            double n0, n1, n2;
            if (wa >= min_weight && wb >= min_weight && (sa < 0) != (sb < 0) &&
                tsdf_edge_normal(t, min_weight, ka, wa, sa, kb, wb, sb, v.dir == 1 ? 0 : v.dir == 2 ? 1 : v.dir == 4 ? 2 : -1, &n0, &n1, &n2)) {
                o0 = (float)n0; o1 = (float)n1; o2 = (float)n2;
                missing = false;
            }
        }
        out[i * 3] = o0; out[i * 3 + 1] = o1; out[i * 3 + 2] = o2;
    }
    const unsigned long long m = __ballot(missing);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(t.head.words + VOXEL_W_OUT, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void tsdf_crossings_kernel(TsdfTable t, uint32_t min_weight, viso_tsdf_crossing* out, unsigned long long out_cap) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;   // the grid covers the slots exactly
    const int lane = threadIdx.x & 63;
    const unsigned long long key = t.head.keys[slot];
    const uint32_t wa = t.weight[slot];
    const bool take = key != MAP_EMPTY && wa >= min_weight;
    if (!__ballot(take)) return;   // the whole wave
    int32_t k[3] = {0, 0, 0};
    long long sa = 0, sb[3] = {0, 0, 0};
    uint32_t wb[3] = {0, 0, 0};
    bool hit[3] = {false, false, false};
    uint32_t mine = 0;
    if (take) {
        voxel_unkey(key, k);
        sa = (long long)t.sum[slot];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (k[ax] == MAP_BIAS - 1) continue;   // the last voxel of the axis has no neighbour
            uint32_t nb;
            if (!voxel_find(t.head.keys, t.head.mask, voxel_neighbour(key, 1u << ax), &nb)) continue;
            wb[ax] = t.weight[nb];
            sb[ax] = (long long)t.sum[nb];
            hit[ax] = wb[ax] >= min_weight && (sa < 0) != (sb[ax] < 0);
            mine += hit[ax] ? 1u : 0u;
        }
    }
    const uint32_t incl = viso_wave_scan(mine);
    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
    if (!total) return;   // the whole wave
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(t.head.words + VOXEL_W_OUT, (unsigned long long)total);
    base = __shfl(base, 0);
    unsigned long long at = base + (incl - mine);
    if (!out) return;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        if (!hit[ax]) continue;
        if (at < out_cap) {
            viso_tsdf_crossing c;
            c.k[0] = k[0]; c.k[1] = k[1]; c.k[2] = k[2];
            c.axis = ax; c.wa = wa; c.wb = wb[ax]; c.sa = sa; c.sb = sb[ax];
            out[at] = c;
        }
        ++at;
    }
}

// ---- triangle mesh by marching tetrahedra (include/viso_hip.h, "TSDF mesh") --------------------------------------
// A cell's corners carry the code c = dx + 2 dy + 4 dz.  Tetrahedron t (the permutations of the axes in lexicographic order) has the
// corners c0 = 0, c1 = c0 + e_pi0, c2 = c1 + e_pi1, c3 = 7: TSDF_TET_CORNERS(t) packs their codes, three bits each.  A tetrahedron's
// case is the four signs of its corners, bit i = corner i negative.  Derived from the rule of the header for the tetrahedron of the
// identity permutation, whose corners are (0,0,0), (1,0,0), (1,1,0), (1,1,1):
//   the number of triangles per case: 0 for none or all negative, 2 for two against two, else 1 (TSDF_TET_COUNTS, two bits a case);
//   the triangles per case: twelve bits a triangle, four a vertex, the vertex on the edge between the local corners i < j as i | j << 2.
//   One corner i alone: e(i, j) over the other corners ascending; N = {a, b}, P = {c, d}: (e(a,c), e(a,d), e(b,d)) and
//   (e(a,c), e(b,d), e(b,c)); the second and third vertex swapped where the normal of the midpoint triangle would point to N.
// The other five tetrahedra are the images of this one under the permutation of the axes, corner i to corner i: a linear map M
// takes (v1 - v0) x (v2 - v0) to det(M) M^-T of it and g to M g, so n . g is multiplied by det(M), the permutation's sign.  The
// same table therefore serves all six, and the odd permutations (tetrahedra 1, 2, 5) swap the second and third vertex once more.
#define TSDF_TET_COUNTS 0x16696994u
#define TSDF_TET_ODD 0x26u
__constant__ uint32_t TSDF_TET_CASES[16] = {0x000000, 0x000c84, 0x0009d4, 0x9d8dc8, 0x000e98, 0xe94ce4, 0x8e4ed4, 0x000edc,
                                            0x000dec, 0xde4e84, 0xec49e4, 0x0009e8, 0xcd8d98, 0x000d94, 0x0008c4, 0x000000};
__device__ __forceinline__ constexpr uint32_t TSDF_TET_CORNERS(int t) {
    return t == 0 ? 0xec8u : t == 1 ? 0xf48u : t == 2 ? 0xed0u : t == 3 ? 0xf90u : t == 4 ? 0xf60u : 0xfa0u;
}

// a triangle as the device lists it: the host sorts by (cell, order) and turns the three (corner, dir) into indices
struct TsdfTriRef {
    unsigned long long cell;   // key of the cell's voxel
    uint32_t code;             // order = 2 tetrahedron + index | v0 << 4 | v1 << 10 | v2 << 16, v = 8 corner code + dir of the edge
    uint32_t pad;
};

// the case of tetrahedron t from the eight signs of the cell (bit c: corner c negative)
__device__ __forceinline__ uint32_t tsdf_tet_case(int t, uint32_t neg) {
    const uint32_t tc = TSDF_TET_CORNERS(t);
    return (neg & 1u) | (((neg >> ((tc >> 3) & 7u)) & 1u) << 1) | (((neg >> ((tc >> 6) & 7u)) & 1u) << 2) | (((neg >> 7) & 1u) << 3);
}

// One thread per slot.  Seven read-only probes for the neighbours at d = 1..7; the voxel's up to seven sign-changing edges as vertex
// records, and, when all eight corners are usable, the cell's up to twelve triangles as references.  verts == null: only the two
// numbers (both lists are written, or neither).
__global__ __launch_bounds__(256) void tsdf_mesh_kernel(TsdfTable t, uint32_t min_weight, double s, viso_tsdf_mesh_vertex* verts,
                                                        unsigned long long v_cap, TsdfTriRef* tris, unsigned long long t_cap) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;   // the grid covers the slots exactly
    const int lane = threadIdx.x & 63;
    const unsigned long long key = t.head.keys[slot];
    const uint32_t wa = t.weight[slot];
    const bool take = key != MAP_EMPTY && wa >= min_weight;
    if (!__ballot(take)) return;   // the whole wave
    int32_t k[3] = {0, 0, 0};
    long long sa = 0, sb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t wb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t usable = 0, neg = 0, hit = 0;   // bit d: the neighbour at d is usable / negative / across a sign change from this voxel
    if (take) {
        voxel_unkey(key, k);
        sa = (long long)t.sum[slot];
        usable = 1u; neg = sa < 0 ? 1u : 0u;
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            // the last voxel of an axis has no neighbour along it: no key is formed beyond a field
            if (((d & 1) && k[0] == MAP_BIAS - 1) || ((d & 2) && k[1] == MAP_BIAS - 1) || ((d & 4) && k[2] == MAP_BIAS - 1)) continue;
            uint32_t nb;
            if (!voxel_find(t.head.keys, t.head.mask, voxel_neighbour(key, d), &nb)) continue;
            wb[d] = t.weight[nb];
            if (wb[d] < min_weight) continue;
            sb[d] = (long long)t.sum[nb];
            usable |= 1u << d;
            if (sb[d] < 0) neg |= 1u << d;
            if ((sb[d] < 0) != (sa < 0)) hit |= 1u << d;
        }
    }
    const bool cell = usable == 0xffu;
    uint32_t n_tri = 0;
    if (cell) {
#pragma unroll
        for (int tet = 0; tet < 6; ++tet) n_tri += (TSDF_TET_COUNTS >> (2u * tsdf_tet_case(tet, neg))) & 3u;
    }
    const uint32_t mine = (uint32_t)__popc(hit) | (n_tri << 16);          // at most 64 x 7 and 64 x 12: both fit 16 bits
    const uint32_t incl = viso_wave_scan(mine);
    const uint32_t total = (uint32_t)__shfl((int)incl, 63);
    if (!total) return;   // the whole wave
    unsigned long long vbase = 0, tbase = 0;
    if (lane == 0) {
        if (total & 0xffffu) vbase = atomicAdd(t.head.words + VOXEL_W_OUT, (unsigned long long)(total & 0xffffu));
        if (total >> 16) tbase = atomicAdd(t.head.words + VOXEL_W_TRIS, (unsigned long long)(total >> 16));
    }
    vbase = __shfl(vbase, 0);
    tbase = __shfl(tbase, 0);
    if (!verts) return;
    unsigned long long at = vbase + ((incl - mine) & 0xffffu);
#pragma unroll
    for (int d = 1; d < 8; ++d) {
        if (!((hit >> d) & 1u)) continue;
        if (at < v_cap) {
            const double da = (double)sa / (double)wa, db = (double)sb[d] / (double)wb[d];
            const double off = da / (da - db) * 1024.0;
            viso_tsdf_mesh_vertex v;
            v.k[0] = k[0]; v.k[1] = k[1]; v.k[2] = k[2];
            v.dir = d;
            v.p[0] = (float)(((double)((long long)k[0] * 1024 + 512) + ((d & 1) ? off : 0.0)) * s);
            v.p[1] = (float)(((double)((long long)k[1] * 1024 + 512) + ((d & 2) ? off : 0.0)) * s);
            v.p[2] = (float)(((double)((long long)k[2] * 1024 + 512) + ((d & 4) ? off : 0.0)) * s);
            v.weight = wa < wb[d] ? wa : wb[d];
            verts[at] = v;
        }
        ++at;
    }
    if (!cell) return;
    at = tbase + ((incl - mine) >> 16);
#pragma unroll
    for (int tet = 0; tet < 6; ++tet) {
        const uint32_t tc = TSDF_TET_CORNERS(tet);
        const uint32_t p = tsdf_tet_case(tet, neg);
        const uint32_t n = (TSDF_TET_COUNTS >> (2u * p)) & 3u;
        if (!n) continue;
        const uint32_t edges = TSDF_TET_CASES[p];
        for (uint32_t q = 0; q < n; ++q) {
            if (at < t_cap) {
                uint32_t v[3];
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const uint32_t e = edges >> (12u * q + 4u * m);
                    const uint32_t ci = (tc >> (3u * (e & 3u))) & 7u, cj = (tc >> (3u * ((e >> 2) & 3u))) & 7u;
                    v[m] = ci * 8u + (cj ^ ci);           // the owner is the corner of the smaller local index; cj's bits include ci's
                }
                const bool odd = (TSDF_TET_ODD >> tet) & 1u;
                TsdfTriRef r;
                r.cell = key;
                r.code = ((uint32_t)(2 * tet) + q) | (v[0] << 4) | ((odd ? v[2] : v[1]) << 10) | ((odd ? v[1] : v[2]) << 16);
                r.pad = 0u;
                tris[at] = r;
            }
            ++at;
        }
    }
}

// ---- ray casting (include/viso_hip.h, "TSDF render") ---------------------------------------------------------------
struct TsdfRenderArgs {
    TsdfTable t;
    const double* poses;               // [views][12] on the device, or null: no transform
    int16_t* disp; uint32_t* weight;   // [views][rows * cols]; weight may be null
    int rows, cols, n_samples; uint32_t min_weight;
    double f, cu, cv, base, s, h;
};

// The body of the render kernels.  GRAY: a run's head lane also loads gray[slot] and hands it to its run, and the hit's intensity
// goes to gray_out; without it, neither pointer is read.  NORMALS: a lane keeps the two voxels of its valid hit, and behind the
// march, where the wave is converged again, the hit's normal in the view's camera frame goes to normals_out [views][px][3]
// (include/viso_hip.h, "TSDF normals"); without it, nothing is kept and the pointer is not read.
template <bool GRAY, bool NORMALS>
__device__ __forceinline__ void tsdf_render_body(const TsdfRenderArgs& a, const unsigned long long* gray, uint8_t* gray_out, float* normals_out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, px = (size_t)a.rows * a.cols;
    const int lane = threadIdx.x & 63, view = blockIdx.y;
    bool march = i < px;
    if (!__ballot(march)) return;   // the whole wave
    const int y = (int)(i / (size_t)a.cols), x = (int)(i - (size_t)y * a.cols);
    const double ra = ((double)x - a.cu) / a.f, rb = ((double)y - a.cv) / a.f;
    // without a pose the identity, as in tsdf_fuse_kernel
    double T0 = 1.0, T1 = 0.0, T2 = 0.0, T3 = 0.0, T4 = 0.0, T5 = 1.0, T6 = 0.0, T7 = 0.0, T8 = 0.0, T9 = 0.0, T10 = 1.0, T11 = 0.0;
    if (a.poses) {
        const double* T = a.poses + (size_t)view * 12;
        T0 = T[0]; T1 = T[1]; T2 = T[2]; T3 = T[3]; T4 = T[4]; T5 = T[5]; T6 = T[6]; T7 = T[7]; T8 = T[8]; T9 = T[9]; T10 = T[10]; T11 = T[11];
    }
    // the previous element of the ray's voxel sequence: its key (empty: none, or a gap since), and where it is usable its payload
    unsigned long long prev = MAP_EMPTY;
    int pkx = 0, pky = 0, pkz = 0;
    uint32_t pw = 0;                   // 0: not usable
    long long ps = 0;
    unsigned long long pg = 0;
    int16_t out_d = VISO_DISP_INVALID;
    uint32_t out_w = 0;
    uint8_t out_g = 0;
    unsigned long long hit_a = MAP_EMPTY, hit_b = MAP_EMPTY;   // NORMALS: the voxels of the valid hit, their weights and sums
    uint32_t hit_wa = 0, hit_wb = 0;
    long long hit_sa = 0, hit_sb = 0;
    for (int n = 1; n <= a.n_samples; ++n) {   // the same n in every lane
        if (!__ballot(march)) break;           // the whole wave
        unsigned long long key = MAP_EMPTY;    // the voxel this lane enters with this sample
        int kx = 0, ky = 0, kz = 0;
        if (march) {
            const double z = (double)n * a.h;
            const double c0 = ra * z, c1 = rb * z;
            const double gx = floor((((T0 * c0 + T1 * c1) + T2 * z) + T3) / a.s);
            const double gy = floor((((T4 * c0 + T5 * c1) + T6 * z) + T7) / a.s);
            const double gz = floor((((T8 * c0 + T9 * c1) + T10 * z) + T11) / a.s);
            if (fabs(gx) < MAP_RANGE && fabs(gy) < MAP_RANGE && fabs(gz) < MAP_RANGE) {   // false for a NaN
                kx = (int)gx >> 10; ky = (int)gy >> 10; kz = (int)gz >> 10;
                const unsigned long long k = voxel_key(kx, ky, kz);
                if (k != prev) key = k;
            } else {
                prev = MAP_EMPTY;              // a gap
                pw = 0;
            }
        }
        if (!__ballot(key != MAP_EMPTY)) continue;   // the whole wave
        // the runs of equal keys along the wave (lanes that enter no voxel: runs of the empty key, which probe nothing)
        bool head;
        uint32_t len;
        voxel_runs(key, lane, &head, &len);
        const int from = voxel_run_head(head, lane);
        uint32_t w = 0;                        // 0: not in the table
        long long sum = 0;
        unsigned long long gs = 0;
        if (head && key != MAP_EMPTY) {
            uint32_t slot;
            if (voxel_find(a.t.head.keys, a.t.head.mask, key, &slot)) {
                w = a.t.weight[slot];
                sum = (long long)a.t.sum[slot];
                if (GRAY) gs = gray[slot];
            }
        }
        w = (uint32_t)__shfl((int)w, from);
        sum = __shfl(sum, from);
        if (GRAY) gs = __shfl(gs, from);
        if (key == MAP_EMPTY) continue;
        if (w < a.min_weight) w = 0;           // (min_weight >= 1: a voxel that is not in the table is not usable either)
        if (w && sum < 0 && prev != MAP_EMPTY && pw && ps >= 0) {
            // the hit: between the centres of the previous voxel and this one
            const double A0 = (double)(pkx * 1024 + 512) * a.s, A1 = (double)(pky * 1024 + 512) * a.s, A2 = (double)(pkz * 1024 + 512) * a.s;
            const double B0 = (double)(kx * 1024 + 512) * a.s, B1 = (double)(ky * 1024 + 512) * a.s, B2 = (double)(kz * 1024 + 512) * a.s;
            const double za = (T2 * (A0 - T3) + T6 * (A1 - T7)) + T10 * (A2 - T11);
            const double zb = (T2 * (B0 - T3) + T6 * (B1 - T7)) + T10 * (B2 - T11);
            const double da = (double)ps / (double)pw, db = (double)sum / (double)w;
            const double t = da / (da - db);
            const double zs = za + (zb - za) * t;
            const double v = ((a.f * a.base) / zs) * 16.0 + 0.5;
            if (zs > 0.0 && v >= 1.0 && !(v >= 32768.0)) {   // false for a NaN
                out_d = (int16_t)(int)floor(v);
                out_w = pw < w ? pw : w;
                if (GRAY) out_g = tsdf_edge_gray(pw, ps, pg, w, sum, gs);
                if (NORMALS) { hit_a = prev; hit_b = key; hit_wa = pw; hit_wb = w; hit_sa = ps; hit_sb = sum; }
            }
            march = false;
        } else {
            prev = key; pkx = kx; pky = ky; pkz = kz; pw = w; ps = sum;
            if (GRAY) pg = gs;
        }
    }
    if (i < px) {
        a.disp[(size_t)view * px + i] = out_d;
        if (a.weight) a.weight[(size_t)view * px + i] = out_w;
        if (GRAY) gray_out[(size_t)view * px + i] = out_g;
    }
    if (NORMALS) {
        float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f;
        double n0, n1, n2;
        if (out_d != VISO_DISP_INVALID && tsdf_edge_normal(a.t, a.min_weight, hit_a, hit_wa, hit_sa, hit_b, hit_wb, hit_sb, -1, &n0, &n1, &n2)) {
            if (a.poses) {   // into the view's camera frame: the rotation's transpose
                o0 = (float)((T0 * n0 + T4 * n1) + T8 * n2);
                o1 = (float)((T1 * n0 + T5 * n1) + T9 * n2);
                o2 = (float)((T2 * n0 + T6 * n1) + T10 * n2);
            } else {
                o0 = (float)n0; o1 = (float)n1; o2 = (float)n2;
            }
        }
        if (i < px) {
            float* o = normals_out + ((size_t)view * px + i) * 3;
            o[0] = o0; o[1] = o1; o[2] = o2;
        }
    }
}

struct TsdfGrayRenderArgs {
    TsdfRenderArgs a;
    const unsigned long long* gray; uint8_t* out;   // the table's sums of intensities; [views][rows * cols]
};

struct TsdfNormalRenderArgs {
    TsdfRenderArgs a;
    float* out;                                     // [views][rows * cols][3]
};

__global__ __launch_bounds__(256) void tsdf_render_kernel(TsdfRenderArgs a) { tsdf_render_body<false, false>(a, nullptr, nullptr, nullptr); }
__global__ __launch_bounds__(256) void tsdf_gray_render_kernel(TsdfGrayRenderArgs g) { tsdf_render_body<true, false>(g.a, g.gray, g.out, nullptr); }
__global__ __launch_bounds__(256) void tsdf_normal_render_kernel(TsdfNormalRenderArgs g) { tsdf_render_body<false, true>(g.a, nullptr, nullptr, g.out); }

// what is in a slot, for the shared kernels that list, zero, add to and evict slots (voxel_hash.h, "a kind's payload"): a plain
// map's, and with GRAY a gray map's, whose table and entries carry the sums of intensities
template <bool GRAY>
struct TsdfPayload {
    std::conditional_t<GRAY, TsdfGrayTable, TsdfTable> tab;
    using Entry = std::conditional_t<GRAY, viso_tsdf_gray_entry, viso_tsdf_entry>;
    static constexpr int UNITS_STAT = VOXEL_ST_UPDATES;   // add_entries: an entry's weight to n_updates,
    static constexpr bool ENTRY_STAT = false;             // and nothing more an entry
    __host__ __device__ __forceinline__ const TsdfTable& t() const { if constexpr (GRAY) return tab.t; else return tab; }
    __host__ __device__ __forceinline__ const VoxelTable& head() const { return t().head; }
    __device__ __forceinline__ uint32_t threshold(uint32_t slot) const { return t().weight[slot]; }
    __device__ __forceinline__ static unsigned long long key(const Entry& v) { return voxel_key(v.k[0], v.k[1], v.k[2]); }
    __device__ __forceinline__ static unsigned long long units(const Entry& v) { return v.weight; }
    __device__ __forceinline__ void add(uint32_t slot, const Entry& v) const {
        atomicAdd(t().weight + slot, v.weight);
        atomicAdd(t().sum + slot, (unsigned long long)v.sum);
        if constexpr (GRAY) atomicAdd(tab.gray + slot, v.gray);
    }
    __device__ __forceinline__ void pack(uint32_t slot, unsigned long long key, uint32_t weight, Entry* v) const {
        voxel_unkey(key, v->k);
        v->weight = weight;
        v->sum = (long long)t().sum[slot];
        if constexpr (GRAY) v->gray = tab.gray[slot];
    }
    __device__ __forceinline__ void zero(uint32_t a) const {
        t().weight[a] = 0u; t().sum[a] = 0ull;
        if constexpr (GRAY) tab.gray[a] = 0ull;
    }
    // a retract's check: nothing but the weight in the slot; and, of a slot of weight w >= 1, what tsdf_add_entries asks of an entry
    // (lim = T 1024 <= 2^13 and w < 2^32: the products fit 64 bits)
    __device__ __forceinline__ bool is_zero(uint32_t a) const {
        if constexpr (GRAY) return t().sum[a] == 0ull && tab.gray[a] == 0ull; else return t().sum[a] == 0ull;
    }
    __device__ __forceinline__ bool within(uint32_t a, uint32_t w, long long lim) const {
        const long long s = (long long)t().sum[a], m = lim * (long long)w;
        if constexpr (GRAY) return s <= m && s >= -m && tab.gray[a] <= 255ull * w; else return s <= m && s >= -m;
    }
    __device__ __forceinline__ void move(uint32_t a, uint32_t b) const {
        t().weight[b] = t().weight[a]; t().sum[b] = t().sum[a];
        if constexpr (GRAY) tab.gray[b] = tab.gray[a];
        zero(a);
    }
};

// ---- host: what is the TSDF map's own; the rest is the shared layer's (voxel_host.h) ----------------------------------------------
struct viso_tsdf {
    VoxelHost h;
    viso_tsdf_params p; double s, hs;        // hs: half a voxel, the step along a ray
    TsdfTable t;                             // the payload in h's block: sum | weight; a gray map's: sum | gray | weight
    unsigned long long* gray;                // null: a plain map
    TsdfFuseOpts o;                          // the map's fuse options, checked; read and written under h.mu
    TsdfGrayTable g() const { return TsdfGrayTable{t, gray}; }
};

// t's payload for the shared kernels; t is live and, with GRAY, a gray map
template <bool GRAY>
static TsdfPayload<GRAY> tsdf_payload(const viso_tsdf* t) {
    if constexpr (GRAY) return {t->g()}; else return {t->t};
}

static VoxelRegistry g_tsdfs = {{"TSDF", "TSDF map", "updates", "min_weight", "viso_tsdf_clear"}};

VoxelRegistry& tsdf_registry() { return g_tsdfs; }
void tsdf_view(viso_tsdf* t, TsdfView* out) {
    out->t = t->t; out->gray = t->gray; out->voxel = t->p.voxel; out->s = t->s; out->trunc_voxels = t->p.trunc_voxels;
}

static bool tsdf_params_ok(const viso_tsdf_params* p) {
    return p && std::isfinite(p->voxel) && p->voxel > 0.0 && p->trunc_voxels >= 1 && p->trunc_voxels <= 8 && p->min_disp16 >= 1 &&
           p->capacity_log2 >= 10 && p->capacity_log2 <= 28;
}

extern "C" void viso_tsdf_params_default(viso_tsdf_params* p) {
    if (!p) return;
    p->voxel = 0.2; p->trunc_voxels = 3; p->min_disp16 = 16; p->capacity_log2 = 26;
}

// the launches the shared layer asks for; t is live by then
static dim3 tsdf_slot_grid(const viso_tsdf* t) { return dim3((t->t.head.mask + 1u) / 256u); }
static VoxelLaunch tsdf_clear_launch(viso_tsdf* t) {
    return [t](hipStream_t s) {
        if (t->gray) voxel_start_clear(tsdf_payload<true>(t), s);
        else voxel_start_clear(tsdf_payload<false>(t), s);
    };
}
// ifs: the distance of two frames' images, for a gray map's fuse (whose calls all come with an image); a plain map's fuse ignores it.
// The map's fuse options are read when a group is launched, under the map's lock (voxel_fuse holds it): at their defaults the
// kernels of before the options, otherwise the extended ones.
static VoxelFuseLaunch tsdf_fuse_launch(viso_tsdf* t, size_t ifs) {
    return [t, ifs](const VoxelFuseArgs& v, const uint8_t* d_image, dim3 grid, hipStream_t s) {
        TsdfFuseArgs a;
        a.v = v; a.trunc = t->p.trunc_voxels; a.s = t->s; a.h = t->hs; a.t = t->t;
        const TsdfFuseOpts o = t->o;
        const bool ext = o.carve > 0 || o.weight_shift >= 0;
        if (d_image) {
            TsdfGrayFuseArgs g;
            g.a = a; g.image = d_image; g.ifs = ifs; g.gray = t->gray;
            if (ext) hipLaunchKernelGGL(tsdf_gray_carve_fuse_kernel, grid, dim3(256), 0, s, g, o);
            else hipLaunchKernelGGL(tsdf_gray_fuse_kernel, grid, dim3(256), 0, s, g);
        } else {
            if (ext) hipLaunchKernelGGL(tsdf_carve_fuse_kernel, grid, dim3(256), 0, s, a, o);
            else hipLaunchKernelGGL(tsdf_fuse_kernel, grid, dim3(256), 0, s, a);
        }
    };
}

// The same for a retract's take (undo: with the sums going back in): the take kernel of the fuse kernel that tsdf_fuse_launch would
// pick, with the map's options as they are when the group is launched.
static VoxelFuseLaunch tsdf_take_launch(viso_tsdf* t, size_t ifs, bool undo) {
    return [t, ifs, undo](const VoxelFuseArgs& v, const uint8_t* d_image, dim3 grid, hipStream_t s) {
        TsdfFuseArgs a;
        a.v = v; a.trunc = t->p.trunc_voxels; a.s = t->s; a.h = t->hs; a.t = t->t;
        const TsdfFuseOpts o = t->o;
        const bool ext = o.carve > 0 || o.weight_shift >= 0;
        if (d_image) {
            TsdfGrayFuseArgs g;
            g.a = a; g.image = d_image; g.ifs = ifs; g.gray = t->gray;
            if (ext) hipLaunchKernelGGL(tsdf_gray_carve_take_kernel, grid, dim3(256), 0, s, g, o, undo);
            else hipLaunchKernelGGL(tsdf_gray_take_kernel, grid, dim3(256), 0, s, g, undo);
        } else {
            if (ext) hipLaunchKernelGGL(tsdf_carve_take_kernel, grid, dim3(256), 0, s, a, o, undo);
            else hipLaunchKernelGGL(tsdf_take_kernel, grid, dim3(256), 0, s, a, undo);
        }
    };
}

static const TsdfFuseOpts TSDF_FUSE_DEFAULTS = {0, -1, 255u, 0, 0.0};

// The values are checked first, on the host alone; then the handle, under the registry's rules.  Either kind of map.
extern "C" int viso_tsdf_set_fuse_options(viso_tsdf* t, int32_t carve_voxels, int32_t weight_shift, uint32_t weight_max, double carve_near) {
    const char* where = "viso_tsdf_set_fuse_options";
    if (carve_voxels < 0 || carve_voxels > 1024 || weight_shift < -1 || weight_shift > 30 || (weight_shift >= 0 && (weight_max < 1 || weight_max > 255)) ||
        !std::isfinite(carve_near) || !(carve_near >= 0.0)) {
        viso_set_error("%s: bad argument (carve_voxels in 0..1024, weight_shift in -1..30, weight_max in 1..255 when weight_shift >= 0, "
                       "a finite carve_near >= 0)", where);
        return VISO_ERR_ARG;
    }
    VoxelSession ses(where, g_tsdfs, t, VoxelSession::ANY_STATE);
    VISO_TRY(ses.status());
    t->o = TsdfFuseOpts{carve_voxels, weight_shift, weight_max, 0, carve_near};
    return VISO_OK;
}

extern "C" int viso_tsdf_get_fuse_options(viso_tsdf* t, int32_t* carve_voxels, int32_t* weight_shift, uint32_t* weight_max, double* carve_near) {
    const char* where = "viso_tsdf_get_fuse_options";
    if (!voxel_known(g_tsdfs, t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    if (!carve_voxels || !weight_shift || !weight_max || !carve_near) { viso_set_error("%s: bad argument (non-null outputs)", where); return VISO_ERR_ARG; }
    VoxelSession ses(where, g_tsdfs, t, VoxelSession::ANY_STATE);
    VISO_TRY(ses.status());
    *carve_voxels = t->o.carve; *weight_shift = t->o.weight_shift; *weight_max = t->o.weight_max; *carve_near = t->o.carve_near;
    return VISO_OK;
}

static int tsdf_create(const char* where, bool gray, viso_ctx* ctx_or_null, const viso_tsdf_params* params, viso_tsdf** out) {
    if (out) *out = nullptr;
    if (!out || !tsdf_params_ok(params)) {
        viso_set_error("%s: bad argument (a finite voxel > 0, trunc_voxels in 1..8, min_disp16 >= 1, capacity_log2 in 10..28, a non-null output)", where);
        return VISO_ERR_ARG;
    }
    viso_tsdf* t = new viso_tsdf();
    char* payload;
    int r = voxel_create(where, g_tsdfs, ctx_or_null, params->capacity_log2, params->min_disp16, gray ? 20 : 12, &t->h, &payload);
    if (r >= 0) {
        const size_t slots = (size_t)1 << params->capacity_log2;
        t->p = *params; t->s = params->voxel / 1024.0; t->hs = params->voxel * 0.5;
        t->t.head = t->h.head;
        t->t.sum = reinterpret_cast<unsigned long long*>(payload); payload += 8 * slots;
        t->gray = nullptr;
        t->o = TSDF_FUSE_DEFAULTS;
        if (gray) { t->gray = reinterpret_cast<unsigned long long*>(payload); payload += 8 * slots; }
        t->t.weight = reinterpret_cast<uint32_t*>(payload);
        r = voxel_open(g_tsdfs, t, &t->h, tsdf_clear_launch(t));
    }
    if (r < 0) { delete t; return r; }
    *out = t;
    return VISO_OK;
}

extern "C" int viso_tsdf_create(viso_ctx* ctx_or_null, const viso_tsdf_params* params, viso_tsdf** out) {
    return tsdf_create("viso_tsdf_create", false, ctx_or_null, params, out);
}
extern "C" int viso_tsdf_create_gray(viso_ctx* ctx_or_null, const viso_tsdf_params* params, viso_tsdf** out) {
    return tsdf_create("viso_tsdf_create_gray", true, ctx_or_null, params, out);
}

// A live handle of the kind the call is for (gray: a gray map), checked before anything else of the call: the kinds do not mix.
static bool tsdf_kind_ok(const char* where, viso_tsdf* t, bool gray) {
    if (!voxel_known(g_tsdfs, t)) { viso_set_error("%s: not a live TSDF handle", where); return false; }
    if ((t->gray != nullptr) != gray) {
        viso_set_error(gray ? "%s: the TSDF map carries no intensity (viso_tsdf_create_gray makes one that does)"
                            : "%s: the TSDF map carries intensity: its calls are the *_gray ones", where);
        return false;
    }
    return true;
}

extern "C" int viso_tsdf_is_gray(viso_tsdf* t, int* out) {
    if (!voxel_known(g_tsdfs, t)) { viso_set_error("viso_tsdf_is_gray: not a live TSDF handle"); return VISO_ERR_ARG; }
    if (!out) { viso_set_error("viso_tsdf_is_gray: bad argument (a non-null output)"); return VISO_ERR_ARG; }
    *out = t->gray ? 1 : 0;
    return VISO_OK;
}

extern "C" int viso_tsdf_destroy(viso_tsdf* t) {
    if (!t) return VISO_OK;
    if (!voxel_unregister("viso_tsdf_destroy", g_tsdfs, t)) return VISO_ERR_ARG;
    const int r = voxel_free("viso_tsdf_destroy", &t->h);
    delete t;
    return r;
}

extern "C" int viso_tsdf_clear(viso_tsdf* t) { return voxel_clear("viso_tsdf_clear", g_tsdfs, t, tsdf_clear_launch(t)); }

int tsdf_is_gray(viso_tsdf* t) { return voxel_known(g_tsdfs, t) && t->gray ? 1 : 0; }

int tsdf_fuse_resident(const char* where, viso_tsdf* t, const DispView& v) {
    if (!tsdf_kind_ok(where, t, v.image != nullptr)) return VISO_ERR_ARG;
    return voxel_fuse(where, g_tsdfs, t, v, tsdf_fuse_launch(t, v.ifs));
}

extern "C" int viso_tsdf_fuse(viso_tsdf* t, const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_or_null) {
    if (!tsdf_kind_ok("viso_tsdf_fuse", t, false)) return VISO_ERR_ARG;
    const DispView v = disp_view_host(disp, nullptr, rows, cols, param, pose_or_null);
    return voxel_fuse("viso_tsdf_fuse", g_tsdfs, t, v, tsdf_fuse_launch(t, v.ifs));
}

extern "C" int viso_tsdf_fuse_gray(viso_tsdf* t, const int16_t* disp, const uint8_t* image, int rows, int cols, const viso_param* param,
                                   const double* pose_or_null) {
    const char* where = "viso_tsdf_fuse_gray";
    if (!tsdf_kind_ok(where, t, true)) return VISO_ERR_ARG;
    if (!image) { viso_set_error("%s: bad argument (a non-null image)", where); return VISO_ERR_ARG; }
    const DispView v = disp_view_host(disp, image, rows, cols, param, pose_or_null);
    return voxel_fuse(where, g_tsdfs, t, v, tsdf_fuse_launch(t, v.ifs));
}

// ---- retract and move (include/viso_hip.h, "TSDF retract") --------------------------------------------------------
// viso_tsdf_retract*, viso_tsdf_move* and the batch's two over the view v of the frames as they were fused (a gray map's with their
// images); move: fused again at poses_new ([v.n][16] or null) behind the retract.  The kind is checked as the fuse calls check it.
int tsdf_retract_resident(const char* where, viso_tsdf* t, const DispView& v, bool move, const double* poses_new, uint64_t* report) {
    if (!tsdf_kind_ok(where, t, v.image != nullptr)) return VISO_ERR_ARG;
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the report's words");
    unsigned long long* rep = reinterpret_cast<unsigned long long*>(report);
    const VoxelRetractLaunches L = {tsdf_take_launch(t, v.ifs, false), tsdf_take_launch(t, v.ifs, true), tsdf_fuse_launch(t, v.ifs),
                                    (long long)t->p.trunc_voxels * 1024};
    if (v.image) return voxel_retract(where, g_tsdfs, t, v, move, poses_new, L, tsdf_payload<true>(t), rep);
    return voxel_retract(where, g_tsdfs, t, v, move, poses_new, L, tsdf_payload<false>(t), rep);
}

extern "C" int viso_tsdf_retract(viso_tsdf* t, const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_or_null,
                                 uint64_t report_or_null[6]) {
    return tsdf_retract_resident("viso_tsdf_retract", t, disp_view_host(disp, nullptr, rows, cols, param, pose_or_null), false, nullptr, report_or_null);
}
extern "C" int viso_tsdf_move(viso_tsdf* t, const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_old_or_null,
                              const double* pose_new_or_null, uint64_t report_or_null[6]) {
    return tsdf_retract_resident("viso_tsdf_move", t, disp_view_host(disp, nullptr, rows, cols, param, pose_old_or_null), true, pose_new_or_null,
                                 report_or_null);
}
// the gray twins: the image the frame was fused with
static int tsdf_retract_gray(const char* where, viso_tsdf* t, const int16_t* disp, const uint8_t* image, int rows, int cols, const viso_param* param,
                             const double* pose, bool move, const double* pose_new, uint64_t* report) {
    if (!tsdf_kind_ok(where, t, true)) return VISO_ERR_ARG;
    if (!image) { viso_set_error("%s: bad argument (a non-null image)", where); return VISO_ERR_ARG; }
    return tsdf_retract_resident(where, t, disp_view_host(disp, image, rows, cols, param, pose), move, pose_new, report);
}
extern "C" int viso_tsdf_retract_gray(viso_tsdf* t, const int16_t* disp, const uint8_t* image, int rows, int cols, const viso_param* param,
                                      const double* pose_or_null, uint64_t report_or_null[6]) {
    return tsdf_retract_gray("viso_tsdf_retract_gray", t, disp, image, rows, cols, param, pose_or_null, false, nullptr, report_or_null);
}
extern "C" int viso_tsdf_move_gray(viso_tsdf* t, const int16_t* disp, const uint8_t* image, int rows, int cols, const viso_param* param,
                                   const double* pose_old_or_null, const double* pose_new_or_null, uint64_t report_or_null[6]) {
    return tsdf_retract_gray("viso_tsdf_move_gray", t, disp, image, rows, cols, param, pose_old_or_null, true, pose_new_or_null, report_or_null);
}

// the checks of an entry that both kinds share
static bool tsdf_entry_ok(const int32_t* k, uint32_t weight, long long sum, long long lim) {
    bool ok = weight >= 1 && sum <= lim * (long long)weight && sum >= -lim * (long long)weight;
    for (int i = 0; i < 3; ++i) ok = ok && k[i] >= -MAP_BIAS && k[i] < MAP_BIAS;
    return ok;
}

// viso_tsdf_add_entries and, with GRAY, viso_tsdf_add_gray_entries
template <bool GRAY>
static int tsdf_add_entries(const char* where, viso_tsdf* t, const typename TsdfPayload<GRAY>::Entry* entries, size_t n) {
    if (!tsdf_kind_ok(where, t, GRAY)) return VISO_ERR_ARG;
    if (n && !entries) { viso_set_error("%s: bad argument (null entries)", where); return VISO_ERR_ARG; }
    const long long lim = (long long)t->p.trunc_voxels * 1024;
    for (size_t i = 0; i < n; ++i) {
        const auto& e = entries[i];
        bool ok = tsdf_entry_ok(e.k, e.weight, e.sum, lim);
        if constexpr (GRAY) ok = ok && e.gray <= 255ull * e.weight;
        if (!ok) {
            viso_set_error("%s: entry %zu is not a voxel of this map (k in -2^20 .. 2^20 - 1, weight >= 1, |sum| <= %lld weight%s)", where, i, lim,
                           GRAY ? ", gray <= 255 weight" : "");
            return VISO_ERR_ARG;
        }
    }
    return voxel_add_entries(where, g_tsdfs, t, entries, n, tsdf_payload<GRAY>(t));
}
extern "C" int viso_tsdf_add_entries(viso_tsdf* t, const viso_tsdf_entry* entries, size_t n) {
    return tsdf_add_entries<false>("viso_tsdf_add_entries", t, entries, n);
}
extern "C" int viso_tsdf_add_gray_entries(viso_tsdf* t, const viso_tsdf_gray_entry* entries, size_t n) {
    return tsdf_add_entries<true>("viso_tsdf_add_gray_entries", t, entries, n);
}

static inline unsigned long long key_of(const int32_t* k) { return voxel_key(k[0], k[1], k[2]); }
static inline bool voxel_item_less(const viso_tsdf_entry& x, const viso_tsdf_entry& y) { return key_of(x.k) < key_of(y.k); }
static inline bool voxel_item_less(const viso_tsdf_gray_entry& x, const viso_tsdf_gray_entry& y) { return key_of(x.k) < key_of(y.k); }
static inline bool voxel_item_less(const viso_tsdf_crossing& x, const viso_tsdf_crossing& y) {
    const unsigned long long a = key_of(x.k), b = key_of(y.k);
    return a != b ? a < b : x.axis < y.axis;
}

// the count or the sorted list of the voxels of at least min_weight updates, as plain entries or, with GRAY, as a gray map's
template <bool GRAY>
static int tsdf_entries(const char* where, viso_tsdf* t, uint32_t min_weight, const VoxelList<typename TsdfPayload<GRAY>::Entry>& list) {
    if (GRAY ? !tsdf_kind_ok(where, t, true) : !voxel_known(g_tsdfs, t)) {
        if (!GRAY) viso_set_error("%s: not a live TSDF handle", where);
        return VISO_ERR_ARG;
    }
    return voxel_entries(where, g_tsdfs, t, min_weight, list, tsdf_payload<GRAY>(t));
}
extern "C" int viso_tsdf_count(viso_tsdf* t, uint32_t min_weight, size_t* n) {   // either kind
    return tsdf_entries<false>("viso_tsdf_count", t, min_weight, {true, nullptr, 0, n});
}
extern "C" int viso_tsdf_get(viso_tsdf* t, uint32_t min_weight, viso_tsdf_entry* entries_out, size_t n_cap, size_t* n) {
    return tsdf_entries<false>("viso_tsdf_get", t, min_weight, {false, entries_out, n_cap, n});
}
extern "C" int viso_tsdf_get_gray(viso_tsdf* t, uint32_t min_weight, viso_tsdf_gray_entry* entries_out, size_t n_cap, size_t* n) {
    return tsdf_entries<true>("viso_tsdf_get_gray", t, min_weight, {false, entries_out, n_cap, n});
}

// viso_tsdf_evict*: t is live and of the payload's kind
template <bool GRAY>
static int tsdf_evict(const char* where, viso_tsdf* t, const viso_voxel_box* keep, const VoxelList<typename TsdfPayload<GRAY>::Entry>& list) {
    return voxel_evict(where, g_tsdfs, t, keep, list, tsdf_payload<GRAY>(t));
}
extern "C" int viso_tsdf_evict_count(viso_tsdf* t, const viso_voxel_box* keep, size_t* n) {   // either kind
    const char* where = "viso_tsdf_evict_count";
    if (!voxel_known(g_tsdfs, t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    return t->gray ? tsdf_evict<true>(where, t, keep, {true, nullptr, 0, n}) : tsdf_evict<false>(where, t, keep, {true, nullptr, 0, n});
}
extern "C" int viso_tsdf_evict(viso_tsdf* t, const viso_voxel_box* keep, viso_tsdf_entry* evicted_out, size_t n_cap, size_t* n) {
    if (!tsdf_kind_ok("viso_tsdf_evict", t, false)) return VISO_ERR_ARG;
    return tsdf_evict<false>("viso_tsdf_evict", t, keep, {false, evicted_out, n_cap, n});
}
extern "C" int viso_tsdf_evict_gray(viso_tsdf* t, const viso_voxel_box* keep, viso_tsdf_gray_entry* evicted_out, size_t n_cap, size_t* n) {
    if (!tsdf_kind_ok("viso_tsdf_evict_gray", t, true)) return VISO_ERR_ARG;
    return tsdf_evict<true>("viso_tsdf_evict_gray", t, keep, {false, evicted_out, n_cap, n});
}

// the count or the sorted list of the crossings between voxels of at least min_weight updates
static int tsdf_crossings(const char* where, viso_tsdf* t, uint32_t min_weight, const VoxelList<viso_tsdf_crossing>& list) {
    return voxel_extract<viso_tsdf_crossing>(where, g_tsdfs, t, min_weight, list,
                                             [=](viso_tsdf_crossing* d_out, unsigned long long out_cap, hipStream_t s) {
        hipLaunchKernelGGL(tsdf_crossings_kernel, tsdf_slot_grid(t), dim3(256), 0, s, t->t, min_weight, d_out, out_cap);
    });
}
extern "C" int viso_tsdf_surface_count(viso_tsdf* t, uint32_t min_weight, size_t* n) {
    return tsdf_crossings("viso_tsdf_surface_count", t, min_weight, {true, nullptr, 0, n});
}
extern "C" int viso_tsdf_surface(viso_tsdf* t, uint32_t min_weight, viso_tsdf_crossing* crossings_out, size_t n_cap, size_t* n) {
    return tsdf_crossings("viso_tsdf_surface", t, min_weight, {false, crossings_out, n_cap, n});
}

// One pass of the mesh extraction: the numbers of vertex records and of triangles, both lists written when `verts` is set
static int tsdf_mesh_pass(viso_tsdf* t, uint32_t min_weight, viso_tsdf_mesh_vertex* verts, size_t v_cap, TsdfTriRef* tris, size_t t_cap,
                          unsigned long long* nv, unsigned long long* nt) {
    return voxel_pass(&t->h, [&](hipStream_t s) {
        hipLaunchKernelGGL(tsdf_mesh_kernel, tsdf_slot_grid(t), dim3(256), 0, s, t->t, min_weight, t->s, verts,
                           (unsigned long long)v_cap, tris, (unsigned long long)t_cap);
    }, nv, nt);
}

static inline bool vertex_less(const viso_tsdf_mesh_vertex& x, const viso_tsdf_mesh_vertex& y) {
    const unsigned long long a = key_of(x.k), b = key_of(y.k);
    return a != b ? a < b : x.dir < y.dir;
}

// Under the session of t.  Both lists from the device, sorted; the vertices no triangle refers to dropped; the references turned
// into indices.
static int tsdf_mesh_lists(const VoxelSession& ses, viso_tsdf* t, uint32_t min_weight, std::vector<viso_tsdf_mesh_vertex>& verts,
                           std::vector<viso_tsdf_triangle>& tris) {
    const char* where = ses.where();
    verts.clear(); tris.clear();
    unsigned long long nv = 0, nt = 0;
    VISO_TRY(tsdf_mesh_pass(t, min_weight, nullptr, 0, nullptr, 0, &nv, &nt));
    if (!nt) return VISO_OK;   // no triangle: no vertex is referred to
    std::vector<viso_tsdf_mesh_vertex> all((size_t)nv);
    std::vector<TsdfTriRef> refs((size_t)nt);
    const size_t bv = (size_t)nv * sizeof(viso_tsdf_mesh_vertex), bt = (size_t)nt * sizeof(TsdfTriRef);
    VoxelScratch d(ses, bt + bv, "the lists");   // the references | the vertices: the 64-bit word of a reference comes first
    VISO_TRY(d.status());
    TsdfTriRef* dt = d.as<TsdfTriRef>();
    viso_tsdf_mesh_vertex* dv = d.as<viso_tsdf_mesh_vertex>(bt);
    unsigned long long nv2 = 0, nt2 = 0;
    VISO_TRY(tsdf_mesh_pass(t, min_weight, dv, (size_t)nv, dt, (size_t)nt, &nv2, &nt2));
    HIP_TRY(hipMemcpy(all.data(), dv, bv, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(refs.data(), dt, bt, hipMemcpyDeviceToHost));
    VISO_TRY(d.release());   // (the host's part below is the long one)
    if (nv2 != nv || nt2 != nt) { viso_set_error("%s: the table changed between the two passes", where); return VISO_ERR_HIP; }   // (the map's lock rules it out)
    std::sort(all.begin(), all.end(), vertex_less);
    std::sort(refs.begin(), refs.end(), [](const TsdfTriRef& x, const TsdfTriRef& y) { return x.cell != y.cell ? x.cell < y.cell : (x.code & 15u) < (y.code & 15u); });
    // every reference to the position of its vertex in the sorted list
    std::vector<unsigned long long> at((size_t)nt * 3);
    std::vector<unsigned char> used((size_t)nv, 0);
    for (size_t i = 0; i < (size_t)nt; ++i) {
        for (int m = 0; m < 3; ++m) {
            const uint32_t v = (refs[i].code >> (4 + 6 * m)) & 63u, c = v >> 3;
            const unsigned long long key = voxel_neighbour(refs[i].cell, c);
            const int dir = (int)(v & 7u);
            size_t lo = 0, hi = (size_t)nv;
            while (lo < hi) {
                const size_t mid = lo + (hi - lo) / 2;
                const unsigned long long km = key_of(all[mid].k);
                if (km < key || (km == key && all[mid].dir < dir)) lo = mid + 1; else hi = mid;
            }
            if (lo == (size_t)nv || key_of(all[lo].k) != key || all[lo].dir != dir) {
                viso_set_error("%s: a triangle refers to a vertex that is not in the list", where);   // (the definition rules it out)
                return VISO_ERR_HIP;
            }
            at[i * 3 + m] = lo;
            used[lo] = 1;
        }
    }
    std::vector<unsigned long long> index((size_t)nv);
    unsigned long long kept = 0;
    for (size_t i = 0; i < (size_t)nv; ++i) { index[i] = kept; kept += used[i]; }
    if (kept > 0xffffffffull) { viso_set_error("%s: %llu vertices are beyond the 32-bit indices of a triangle", where, kept); return VISO_ERR_UNSUPPORTED; }
    verts.reserve((size_t)kept);
    for (size_t i = 0; i < (size_t)nv; ++i) if (used[i]) verts.push_back(all[i]);
    tris.resize((size_t)nt);
    for (size_t i = 0; i < (size_t)nt; ++i) for (int m = 0; m < 3; ++m) tris[i].v[m] = (uint32_t)index[(size_t)at[i * 3 + m]];
    return VISO_OK;
}

// viso_tsdf_mesh_count (both lists count_only) and viso_tsdf_mesh
static int tsdf_mesh_extract(const char* where, viso_tsdf* t, uint32_t min_weight, const VoxelList<viso_tsdf_mesh_vertex>& v,
                             const VoxelList<viso_tsdf_triangle>& tr) {
    if (!voxel_known(g_tsdfs, t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    if (!v.n || !tr.n || min_weight < 1 || (!v.count_only && ((v.cap && !v.out) || (tr.cap && !tr.out)))) {
        viso_set_error("%s: bad argument (min_weight >= 1, non-null outputs)", where);
        return VISO_ERR_ARG;
    }
    std::vector<viso_tsdf_mesh_vertex> verts;
    std::vector<viso_tsdf_triangle> tris;
    {   // the map's lock is not held over the copies to the caller's arrays
        VoxelSession ses(where, g_tsdfs, t);
        VISO_TRY(ses.status());
        VISO_TRY(tsdf_mesh_lists(ses, t, min_weight, verts, tris));
    }
    *v.n = verts.size();
    *tr.n = tris.size();
    if (v.count_only) return VISO_OK;
    if (verts.size() > v.cap || tris.size() > tr.cap) {
        viso_set_error("%s: %zu vertices and %zu triangles do not fit the %zu and %zu given", where, verts.size(), tris.size(), v.cap, tr.cap);
        return VISO_ERR_ARG;
    }
    std::copy(verts.begin(), verts.end(), v.out);
    std::copy(tris.begin(), tris.end(), tr.out);
    return VISO_OK;
}

extern "C" int viso_tsdf_mesh_count(viso_tsdf* t, uint32_t min_weight, size_t* n_vertices, size_t* n_triangles) {
    return tsdf_mesh_extract("viso_tsdf_mesh_count", t, min_weight, {true, nullptr, 0, n_vertices}, {true, nullptr, 0, n_triangles});
}
extern "C" int viso_tsdf_mesh(viso_tsdf* t, uint32_t min_weight, viso_tsdf_mesh_vertex* vertices_out, size_t nv_cap,
                              viso_tsdf_triangle* triangles_out, size_t nt_cap, size_t* n_vertices, size_t* n_triangles) {
    return tsdf_mesh_extract("viso_tsdf_mesh", t, min_weight, {false, vertices_out, nv_cap, n_vertices}, {false, triangles_out, nt_cap, n_triangles});
}

// the views a render is asked for, and where they go
struct TsdfRenderCall {
    uint32_t min_weight; const viso_param* param; int rows, cols; double max_depth;
    const double* poses_or_null; int n_views;
    VoxelRenderOut out;
};

// viso_tsdf_render (out.gray and out.normals null), viso_tsdf_render_gray and viso_tsdf_render_normals (normals: out.normals set)
static int tsdf_render(const char* where, viso_tsdf* t, bool gray, bool normals, const TsdfRenderCall& c) {
    // what does not need the map first, so that nothing of a wrong call reaches a handle
    if (c.min_weight < 1 || (gray && !c.out.gray) || (normals && !c.out.normals) || !c.param || !c.out.disp || c.rows < 1 || c.cols < 1 || c.n_views < 1 ||
        (!c.poses_or_null && c.n_views != 1) || !(std::isfinite(c.max_depth) && c.max_depth > 0.0)) {
        viso_set_error("%s: bad argument (min_weight >= 1, non-null calibration and output, sizes >= 1, a finite max_depth > 0, n_views >= 1 "
                       "and 1 without poses)", where);
        return VISO_ERR_ARG;
    }
    if (!(std::isfinite(c.param->f) && std::isfinite(c.param->cu) && std::isfinite(c.param->cv) && std::isfinite(c.param->base) && c.param->f > 0.0 &&
          c.param->base > 0.0)) {
        viso_set_error("%s: bad argument (the calibration f, cu, cv, base must be finite, f > 0 and base > 0)", where);
        return VISO_ERR_ARG;
    }
    if ((long long)c.rows * c.cols > VOXEL_MAX_PIXELS) { viso_set_error("%s: bad argument (a %d x %d view is beyond 2^31 - 1 pixels)", where, c.rows, c.cols); return VISO_ERR_ARG; }
    if (c.poses_or_null) {
        for (size_t i = 0; i < (size_t)c.n_views * 16; ++i) {
            if (!std::isfinite(c.poses_or_null[i])) { viso_set_error("%s: bad argument (pose %zu has an entry that is not finite)", where, i / 16); return VISO_ERR_ARG; }
        }
    }
    if (gray ? !tsdf_kind_ok(where, t, true) : !voxel_known(g_tsdfs, t)) {
        if (!gray) viso_set_error("%s: not a live TSDF handle", where);
        return VISO_ERR_ARG;
    }
    const double steps = floor(c.max_depth / t->hs);
    if (!(steps >= 1.0 && steps <= 65536.0)) {
        viso_set_error("%s: bad argument (max_depth %g is %g steps of half a voxel: 1 .. 65536)", where, c.max_depth, steps);
        return VISO_ERR_ARG;
    }
    TsdfRenderArgs a;
    a.t = t->t;
    a.rows = c.rows; a.cols = c.cols; a.n_samples = (int)steps; a.min_weight = c.min_weight;
    a.f = c.param->f; a.cu = c.param->cu; a.cv = c.param->cv; a.base = c.param->base; a.s = t->s; a.h = t->hs;
    const unsigned long long* table_gray = t->gray;
    return voxel_render(where, g_tsdfs, t, (size_t)c.rows * c.cols, c.poses_or_null, c.n_views, c.out,
                        [a, table_gray](const double* d_poses, int16_t* d_disp, uint32_t* d_weight, uint8_t* d_gray, float* d_normals, dim3 grid,
                                        hipStream_t s) {
        TsdfRenderArgs g = a;
        g.poses = d_poses; g.disp = d_disp; g.weight = d_weight;
        if (d_normals) {
            TsdfNormalRenderArgs gn;
            gn.a = g; gn.out = d_normals;
            hipLaunchKernelGGL(tsdf_normal_render_kernel, grid, dim3(256), 0, s, gn);
        } else if (d_gray) {
            TsdfGrayRenderArgs gg;
            gg.a = g; gg.gray = table_gray; gg.out = d_gray;
            hipLaunchKernelGGL(tsdf_gray_render_kernel, grid, dim3(256), 0, s, gg);
        } else {
            hipLaunchKernelGGL(tsdf_render_kernel, grid, dim3(256), 0, s, g);
        }
    });
}

extern "C" int viso_tsdf_render(viso_tsdf* t, uint32_t min_weight, const viso_param* param, int rows, int cols, double max_depth,
                                const double* poses_or_null, int n_views, int16_t* disp_out, uint32_t* weight_out_or_null) {
    return tsdf_render("viso_tsdf_render", t, false, false,
                       {min_weight, param, rows, cols, max_depth, poses_or_null, n_views, {disp_out, weight_out_or_null, nullptr, nullptr}});
}
extern "C" int viso_tsdf_render_gray(viso_tsdf* t, uint32_t min_weight, const viso_param* param, int rows, int cols, double max_depth,
                                     const double* poses_or_null, int n_views, int16_t* disp_out, uint32_t* weight_out_or_null, uint8_t* gray_out) {
    return tsdf_render("viso_tsdf_render_gray", t, true, false,
                       {min_weight, param, rows, cols, max_depth, poses_or_null, n_views, {disp_out, weight_out_or_null, gray_out, nullptr}});
}
extern "C" int viso_tsdf_render_normals(viso_tsdf* t, uint32_t min_weight, const viso_param* param, int rows, int cols, double max_depth,
                                        const double* poses_or_null, int n_views, int16_t* disp_out, uint32_t* weight_out_or_null,
                                        float* normals_out) {
    return tsdf_render("viso_tsdf_render_normals", t, false, true,
                       {min_weight, param, rows, cols, max_depth, poses_or_null, n_views, {disp_out, weight_out_or_null, nullptr, normals_out}});
}

// the (k, dir) of a vertex list, of which nothing else is read: every one an edge of the key range.  Host only.
static bool tsdf_vertices_ok(const char* where, const viso_tsdf_mesh_vertex* vertices, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const viso_tsdf_mesh_vertex& v = vertices[i];
        bool ok = v.dir >= 1 && v.dir <= 7;
        for (int k = 0; k < 3 && ok; ++k) ok = v.k[k] >= -MAP_BIAS && v.k[k] < MAP_BIAS - ((v.dir >> k) & 1);
        if (!ok) {
            viso_set_error("%s: vertex %zu is not an edge of this map (dir in 1..7, k in -2^20 .. 2^20 - 1, and below 2^20 - 1 along dir)", where, i);
            return false;
        }
    }
    return true;
}

// viso_tsdf_vertex_gray and viso_tsdf_vertex_normals behind their own checks: the n vertices to the device, one pass of `launch`
// (a thread a vertex) with out_bytes a vertex of output behind them, the output and the number of vertices without one back.
// (A vertex is a multiple of four bytes, so an output of floats behind the vertices stays aligned.)
using TsdfSampleLaunch = std::function<void(const viso_tsdf_mesh_vertex* d_verts, void* d_out, dim3 grid, hipStream_t)>;
static int tsdf_sample_vertices(const char* where, viso_tsdf* t, const viso_tsdf_mesh_vertex* vertices, size_t n, size_t out_bytes, void* out,
                                size_t* n_missing_or_null, const TsdfSampleLaunch& launch) {
    VoxelSession ses(where, g_tsdfs, t);
    VISO_TRY(ses.status());
    if (n_missing_or_null) *n_missing_or_null = 0;
    if (!n) return VISO_OK;
    const size_t b_verts = n * sizeof(viso_tsdf_mesh_vertex), b_out = n * out_bytes;
    VoxelScratch d(ses, b_verts + b_out, "the vertices");
    VISO_TRY(d.status());
    HIP_TRY(hipMemcpy(d.as<char>(), vertices, b_verts, hipMemcpyHostToDevice));
    unsigned long long missing = 0;
    VISO_TRY(voxel_pass(ses.host(), [&](hipStream_t s) {
        launch(d.as<viso_tsdf_mesh_vertex>(), d.as<char>(b_verts), dim3((unsigned)((n + 255) / 256)), s);
    }, &missing));
    HIP_TRY(hipMemcpy(out, d.as<char>(b_verts), b_out, hipMemcpyDeviceToHost));
    if (n_missing_or_null) *n_missing_or_null = (size_t)missing;
    return VISO_OK;
}

extern "C" int viso_tsdf_vertex_gray(viso_tsdf* t, const viso_tsdf_mesh_vertex* vertices, size_t n, uint8_t* gray_out, size_t* n_missing_or_null) {
    const char* where = "viso_tsdf_vertex_gray";
    if (!tsdf_kind_ok(where, t, true)) return VISO_ERR_ARG;
    if (n && (!vertices || !gray_out)) { viso_set_error("%s: bad argument (non-null vertices and output)", where); return VISO_ERR_ARG; }
    if (!tsdf_vertices_ok(where, vertices, n)) return VISO_ERR_ARG;
    return tsdf_sample_vertices(where, t, vertices, n, 1, gray_out, n_missing_or_null,
                                [=](const viso_tsdf_mesh_vertex* d_verts, void* d_out, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL(tsdf_gray_sample_kernel, grid, dim3(256), 0, s, t->g(), d_verts, (unsigned long long)n, static_cast<uint8_t*>(d_out));
    });
}

extern "C" int viso_tsdf_vertex_normals(viso_tsdf* t, uint32_t min_weight, const viso_tsdf_mesh_vertex* vertices, size_t n, float* normals_out,
                                        size_t* n_missing_or_null) {
    const char* where = "viso_tsdf_vertex_normals";
    // what does not need the map first, so that nothing of a wrong call reaches a handle
    if (min_weight < 1 || (n && (!vertices || !normals_out))) {
        viso_set_error("%s: bad argument (min_weight >= 1, non-null vertices and output)", where);
        return VISO_ERR_ARG;
    }
    if (n > (size_t)-1 / (sizeof(viso_tsdf_mesh_vertex) + 3 * sizeof(float))) {
        viso_set_error("%s: bad argument (%zu vertices are beyond the address space)", where, n);
        return VISO_ERR_ARG;
    }
    if (!tsdf_vertices_ok(where, vertices, n)) return VISO_ERR_ARG;
    if (!voxel_known(g_tsdfs, t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    return tsdf_sample_vertices(where, t, vertices, n, 3 * sizeof(float), normals_out, n_missing_or_null,
                                [=](const viso_tsdf_mesh_vertex* d_verts, void* d_out, dim3 grid, hipStream_t s) {
        hipLaunchKernelGGL(tsdf_normal_sample_kernel, grid, dim3(256), 0, s, t->t, min_weight, d_verts, (unsigned long long)n, static_cast<float*>(d_out));
    });
}

extern "C" int viso_tsdf_stats(viso_tsdf* t, viso_tsdf_counters* out) {
    unsigned long long sums[4], dropped;
    const int r = voxel_stats("viso_tsdf_stats", g_tsdfs, t, out, sums, &dropped);
    if (r < 0) return r;
    out->n_points = sums[VOXEL_ST_POINTS]; out->n_updates = sums[VOXEL_ST_UPDATES]; out->n_out_of_range = sums[VOXEL_ST_OOR];
    out->n_occupied = sums[VOXEL_ST_OCC]; out->n_dropped = dropped;
    return VISO_OK;
}

extern "C" int viso_tsdf_crossing_point(const viso_tsdf_crossing* c, double voxel, float out[3]) {
    if (!c || !out || c->axis < 0 || c->axis > 2 || c->wa < 1 || c->wb < 1 || (c->sa < 0) == (c->sb < 0) || !(std::isfinite(voxel) && voxel > 0.0)) {
        viso_set_error("viso_tsdf_crossing_point: bad argument (non-null crossing and output, axis in 0..2, weights >= 1, sums of "
                       "different sign, a finite voxel > 0)");
        return VISO_ERR_ARG;
    }
    const double s = voxel / 1024.0;
    const double da = (double)c->sa / (double)c->wa, db = (double)c->sb / (double)c->wb;
    const double t = da / (da - db);
    for (int i = 0; i < 3; ++i) {
        const double centre = (double)((long long)c->k[i] * 1024 + 512);
        out[i] = (float)((centre + (i == c->axis ? t * 1024.0 : 0.0)) * s);
    }
    return VISO_OK;
}
