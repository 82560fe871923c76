// tsdf_align.hip — opt-in frame-to-model alignment of a disparity map against a TSDF map (NOT in the reference: viso_tsdf_linearize,
// viso_tsdf_align, viso_batch_align_tsdf; include/viso_hip.h, "TSDF align"), and the same with a photometric row
// from a gray map's sums of intensities (viso_tsdf_linearize_gray, viso_tsdf_align_gray, viso_batch_align_tsdf_gray; "TSDF
// photometric align").  Direct tracking on the signed distance:
// every valid pixel's back-projected point samples the distance trilinearly and contributes one row to a 6 x 6 Gauss-Newton system
// whose entries are sums of integers, so the kernel's output is bit-identical to tests/align_ref.py however the sums are combined.
//
//   tsdf_linearize_kernel   the lanes of a wave take consecutive pixels of a row; a thread strides over `trips` pixels, grid.x * 256
//                           apart, the frames of a round along the grid's y.  Lanes whose cell k0 equals that of the lane to their
//                           left form a run (voxel_runs): only the run's head lane does the eight read-only probes (voxel_find) and
//                           loads, the other lanes take the 8 x (weight, sum lo, sum hi) words from it (24 ds_bpermute), as
//                           tsdf_render_kernel does for one voxel.  Who loads changes, not what is loaded.  The 28 sums are int64
//                           in registers (a pixel that is not used adds zeros); the six counters are wave totals from ballots.  At
//                           the end one DPP reduction per sum (viso_wave_sum63), the four waves' totals through 1088 bytes of LDS,
//                           and threads 0..33 add the workgroup's totals to the frame's 34 words: one 64-bit integer atomic each,
//                           and none for a zero.  A frame whose flag is 0 (its alignment has finished) leaves at once.
//                           No float atomics, no scratch; no workgroup waits for another; every probe loop is the table layer's.
//   tsdf_gray_linearize_kernel   the same body (tsdf_linearize_body<true>): the head lane also loads gray[slot] of its eight voxels
//                           (16 more ds_bpermute), the pixel's byte is read along the row as tsdf_gray_fuse_kernel reads it, the
//                           second row's products add into the same 28 registers without a branch (a row that is not used adds
//                           zeros), p and three counters join the reduction: 38 words a frame, 1216 bytes of LDS.
// The table's layout is tsdf_table.h's, the probes and the runs voxel_hash.h's, the staging of a round voxel_host.h's
// (voxel_linearize); the 6 x 6 solve and the loop are alignmath.cpp's.
#include "common.h"
#include "wave.h"
#include "tsdf_table.h"
#include "alignmath.h"

#include <cmath>
#include <cstring>

#define ALIGN_WORDS 34                  // viso_tsdf_normal: n[28], then the six counters
#define ALIGN_GRAY_WORDS 38             // viso_tsdf_normal_gray: those, then p and the three photometric counters
#define ALIGN_MAX_PIXELS (1ll << 22)
#define ALIGN_BLOCKS 512u               // along x at most: a full KITTI frame is 3.6 pixels a thread

struct TsdfAlignArgs {
    VoxelFuseArgs v;                    // the maps, the poses [frames][12] and the calibration
    TsdfTable t;
    const unsigned long long* active;   // [frames]
    unsigned long long* out;            // [frames][ALIGN_WORDS]; the gray kernel's: [frames][ALIGN_GRAY_WORDS]
    double voxel, s, gate;              // gate: gate_voxels 1024
    uint32_t min_weight; int trips;     // pixels a thread
};

struct TsdfGrayAlignArgs {
    TsdfAlignArgs a;
    const unsigned long long* gray;     // the table's sums of intensities [slots]
    const uint8_t* image; size_t ifs;   // frame f's image at image + f * ifs
    double lambda, photo_gate;
};

// A_i of step 8; *clip set when the value is not finite or beyond 2^20
__device__ __forceinline__ int align_round(double a, bool* clip) {
    const double r = floor(a * 256.0 + 0.5);
    if (!(fabs(r) < 1048576.0)) { *clip = true; return 0; }   // also a NaN
    return (int)r;
}

// step 5 on the eight corners m[dx + 2 dy + 4 dz]: the value and its derivative per voxel along x, y, z
struct AlignSample { double psi, d0, d1, d2; };
__device__ __forceinline__ AlignSample align_interpolate(double m0, double m1, double m2, double m3, double m4, double m5, double m6, double m7,
                                                         double t0, double t1, double t2) {
    // x?_zy is X?[dz][dy]
    const double x1_00 = m1 - m0, x1_01 = m3 - m2, x1_10 = m5 - m4, x1_11 = m7 - m6;
    const double x0_00 = m0 + t0 * x1_00, x0_01 = m2 + t0 * x1_01, x0_10 = m4 + t0 * x1_10, x0_11 = m6 + t0 * x1_11;
    const double y1_0 = x0_01 - x0_00, y1_1 = x0_11 - x0_10;
    const double y0_0 = x0_00 + t1 * y1_0, y0_1 = x0_10 + t1 * y1_1;
    const double yx_0 = x1_00 + t1 * (x1_01 - x1_00), yx_1 = x1_10 + t1 * (x1_11 - x1_10);
    const double d2 = y0_1 - y0_0;
    const double psi = y0_0 + t2 * d2;
    const double d0 = yx_0 + t2 * (yx_1 - yx_0);
    const double d1 = y1_0 + t2 * (y1_1 - y1_0);
    return AlignSample{psi, d0, d1, d2};
}

// The body of both linearise kernels.  GRAY: the run's head lane also loads the gray sums of its eight voxels and hands them to
// its run (16 more ds_bpermute), the pixel's intensity is read along the row, and a used pixel's second row ("TSDF photometric
// align", P1..P6) adds its products into the same 28 sums; p and the three photometric counters join the reduction.
template <bool GRAY>
__device__ __forceinline__ void tsdf_linearize_body(const TsdfAlignArgs& a, const unsigned long long* gray, const uint8_t* image, size_t ifs,
                                                    double lambda, double photo_gate) {
    constexpr int WORDS = GRAY ? ALIGN_GRAY_WORDS : ALIGN_WORDS;
    __shared__ unsigned long long part[4][WORDS];
    const int fr = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!a.active[fr]) return;   // the whole workgroup
    const double* T = a.v.poses + (size_t)fr * 12;
    const double T0 = T[0], T1 = T[1], T2 = T[2], T3 = T[3], T4 = T[4], T5 = T[5], T6 = T[6], T7 = T[7], T8 = T[8], T9 = T[9], T10 = T[10], T11 = T[11];
    const double fb = a.v.f * a.v.base;
    long long N[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) N[k] = 0;
    long long P = 0;   // GRAY: the photometric part of N[27]
    unsigned long long n_points = 0, n_used = 0, n_missing = 0, n_gated = 0, n_clipped = 0, n_oor = 0;   // wave totals
    unsigned long long n_photo_used = 0, n_photo_gated = 0, n_photo_clipped = 0;
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (int trip = 0; trip < a.trips; ++trip, i += stride) {   // the same trip in every lane
        double X = 0.0, Y = 0.0, Z = 1.0;
        const bool point = voxel_point(a.v, i, fr, &X, &Y, &Z);
        double pix = 0.0;
        if (GRAY && point) pix = (double)image[(size_t)fr * ifs + i];   // i is inside the image: voxel_point has checked it
        const unsigned long long pm = __ballot(point);
        if (!pm) continue;   // the whole wave
        n_points += __popcll(pm);
        unsigned long long key = MAP_EMPTY;   // the cell's first voxel k0
        double t0 = 0.0, t1 = 0.0, t2 = 0.0;
        if (point) {
            const double u0 = (((T0 * X + T1 * Y) + T2 * Z) + T3) / a.voxel - 0.5;
            const double u1 = (((T4 * X + T5 * Y) + T6 * Z) + T7) / a.voxel - 0.5;
            const double u2 = (((T8 * X + T9 * Y) + T10 * Z) + T11) / a.voxel - 0.5;
            const double f0 = floor(u0), f1 = floor(u1), f2 = floor(u2);
            // -2^20 .. 2^20 - 2; false for a NaN and for an infinity
            if (f0 >= -1048576.0 && f0 <= 1048574.0 && f1 >= -1048576.0 && f1 <= 1048574.0 && f2 >= -1048576.0 && f2 <= 1048574.0) {
                key = voxel_key((int)f0, (int)f1, (int)f2);
                t0 = u0 - f0; t1 = u1 - f1; t2 = u2 - f2;
            }
        }
        const bool have = key != MAP_EMPTY;
        const unsigned long long hm = __ballot(have);
        n_oor += __popcll(pm & ~hm);
        if (!hm) continue;   // the whole wave
        // the runs of equal cells along the wave (lanes without one: runs of the empty key, which probe nothing)
        bool head;
        uint32_t len;
        voxel_runs(key, lane, &head, &len);
        const int from = voxel_run_head(head, lane);
        uint32_t w[8];
        long long sm[8];
        unsigned long long gr[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) { w[c] = 0u; sm[c] = 0; gr[c] = 0ull; }   // 0: not in the table
        if (head && have) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                uint32_t slot;
                if (voxel_find(a.t.head.keys, a.t.head.mask, voxel_neighbour(key, (uint32_t)c), &slot)) {
                    w[c] = a.t.weight[slot];
                    sm[c] = (long long)a.t.sum[slot];
                    if (GRAY) gr[c] = gray[slot];
                }
            }
        }
        bool usable = have;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            w[c] = (uint32_t)__shfl((int)w[c], from);
            sm[c] = __shfl(sm[c], from);
            if (GRAY) gr[c] = (unsigned long long)__shfl((long long)gr[c], from);
            usable = usable && w[c] >= a.min_weight;   // (min_weight >= 1: a voxel that is not in the table is not usable either)
        }
        n_missing += __popcll(__ballot(have && !usable));
        bool gated = false, clip = false;
        int A0 = 0, A1 = 0, A2 = 0, A3 = 0, A4 = 0, A5 = 0, A6 = 0;
        if (usable) {
            const double m0 = (double)sm[0] / (double)w[0], m1 = (double)sm[1] / (double)w[1], m2 = (double)sm[2] / (double)w[2],
                         m3 = (double)sm[3] / (double)w[3], m4 = (double)sm[4] / (double)w[4], m5 = (double)sm[5] / (double)w[5],
                         m6 = (double)sm[6] / (double)w[6], m7 = (double)sm[7] / (double)w[7];
            const AlignSample ps = align_interpolate(m0, m1, m2, m3, m4, m5, m6, m7, t0, t1, t2);   // the corner dx + 2 dy + 4 dz is m[dz][dy][dx]
            const double psi = ps.psi, d0 = ps.d0, d1 = ps.d1, d2 = ps.d2;
            if (fabs(psi) > a.gate) {
                gated = true;
            } else {
                const double g0 = d0 / 1024.0, g1 = d1 / 1024.0, g2 = d2 / 1024.0;
                const double wt = fb / (Z * Z);
                const double e = (psi * a.s) * wt;
                const double c0 = (T0 * g0 + T4 * g1) + T8 * g2;
                const double c1 = (T1 * g0 + T5 * g1) + T9 * g2;
                const double c2 = (T2 * g0 + T6 * g1) + T10 * g2;
                A0 = align_round(c0 * wt, &clip);
                A1 = align_round(c1 * wt, &clip);
                A2 = align_round(c2 * wt, &clip);
                A3 = align_round((Y * c2 - Z * c1) * wt, &clip);
                A4 = align_round((Z * c0 - X * c2) * wt, &clip);
                A5 = align_round((X * c1 - Y * c0) * wt, &clip);
                A6 = align_round(e, &clip);
            }
        }
        n_gated += __popcll(__ballot(gated));
        n_clipped += __popcll(__ballot(clip));
        const bool used = usable && !gated && !clip;
        n_used += __popcll(__ballot(used));
        const int A[7] = {used ? A0 : 0, used ? A1 : 0, used ? A2 : 0, used ? A3 : 0, used ? A4 : 0, used ? A5 : 0, used ? A6 : 0};
        int at = 0;
#pragma unroll
        for (int p = 0; p < 7; ++p) {
#pragma unroll
            for (int q = p; q < 7; ++q, ++at) N[at] += (long long)A[p] * (long long)A[q];   // |A| < 2^20: below 2^40 each
        }
        if (GRAY) {
            bool pgated = false, pclip = false;
            int B0 = 0, B1 = 0, B2 = 0, B3 = 0, B4 = 0, B5 = 0, B6 = 0;
            if (used) {   // every w[c] >= min_weight >= 1
                const AlignSample is = align_interpolate((double)gr[0] / (double)w[0], (double)gr[1] / (double)w[1], (double)gr[2] / (double)w[2],
                                                         (double)gr[3] / (double)w[3], (double)gr[4] / (double)w[4], (double)gr[5] / (double)w[5],
                                                         (double)gr[6] / (double)w[6], (double)gr[7] / (double)w[7], t0, t1, t2);
                const double e0 = is.d0, e1 = is.d1, e2 = is.d2;
                const double r = is.psi - pix;
                if (fabs(r) > photo_gate) {
                    pgated = true;
                } else {
                    const double h0 = e0 / a.voxel, h1 = e1 / a.voxel, h2 = e2 / a.voxel;
                    const double c0 = (T0 * h0 + T4 * h1) + T8 * h2;
                    const double c1 = (T1 * h0 + T5 * h1) + T9 * h2;
                    const double c2 = (T2 * h0 + T6 * h1) + T10 * h2;
                    B0 = align_round(c0 * lambda, &pclip);
                    B1 = align_round(c1 * lambda, &pclip);
                    B2 = align_round(c2 * lambda, &pclip);
                    B3 = align_round((Y * c2 - Z * c1) * lambda, &pclip);
                    B4 = align_round((Z * c0 - X * c2) * lambda, &pclip);
                    B5 = align_round((X * c1 - Y * c0) * lambda, &pclip);
                    B6 = align_round(r * lambda, &pclip);
                }
            }
            n_photo_gated += __popcll(__ballot(pgated));
            n_photo_clipped += __popcll(__ballot(pclip));
            const bool pused = used && !pgated && !pclip;
            n_photo_used += __popcll(__ballot(pused));
            const int B[7] = {pused ? B0 : 0, pused ? B1 : 0, pused ? B2 : 0, pused ? B3 : 0, pused ? B4 : 0, pused ? B5 : 0, pused ? B6 : 0};
            at = 0;
#pragma unroll
            for (int p = 0; p < 7; ++p) {
#pragma unroll
                for (int q = p; q < 7; ++q, ++at) N[at] += (long long)B[p] * (long long)B[q];   // the second product below 2^40
            }
            P += (long long)B[6] * (long long)B[6];
        }
    }
    // the wave's totals to lane 63, the four waves' through LDS, the workgroup's with one atomic a word
#pragma unroll
    for (int k = 0; k < 28; ++k) {
        const unsigned long long v = viso_wave_sum63((unsigned long long)N[k]);
        if (lane == 63) part[wave][k] = v;
    }
    if (lane == 63) {
        part[wave][28] = n_points; part[wave][29] = n_used; part[wave][30] = n_missing;
        part[wave][31] = n_gated; part[wave][32] = n_clipped; part[wave][33] = n_oor;
    }
    if (GRAY) {
        const unsigned long long v = viso_wave_sum63((unsigned long long)P);
        if (lane == 63) {
            part[wave][34] = v; part[wave][35] = n_photo_used; part[wave][36] = n_photo_gated; part[wave][37] = n_photo_clipped;
        }
    }
    __syncthreads();
    if (threadIdx.x < WORDS) {
        const unsigned long long v = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if (v) atomicAdd(a.out + (size_t)fr * WORDS + threadIdx.x, v);
    }
}

__global__ __launch_bounds__(256) void tsdf_linearize_kernel(TsdfAlignArgs a) { tsdf_linearize_body<false>(a, nullptr, nullptr, 0, 0.0, 0.0); }
__global__ __launch_bounds__(256) void tsdf_gray_linearize_kernel(TsdfGrayAlignArgs g) {
    tsdf_linearize_body<true>(g.a, g.gray, g.image, g.ifs, g.lambda, g.photo_gate);
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------
extern "C" void viso_tsdf_align_params_default(viso_tsdf_align_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->min_weight = 2; p->gate_voxels = 1.0; p->max_iters = 10; p->eps_rot = 1e-6; p->eps_trans = 1e-5; p->min_pixels = 200;
}

// the part of the parameters' check that does not need the map (gate_voxels <= trunc_voxels does)
static bool align_params_ok(const viso_tsdf_align_params* p) {
    return p && p->min_weight >= 1 && std::isfinite(p->gate_voxels) && p->gate_voxels > 0.0 && p->max_iters >= 1 && p->max_iters <= 50 &&
           std::isfinite(p->eps_rot) && p->eps_rot >= 0.0 && std::isfinite(p->eps_trans) && p->eps_trans >= 0.0 && p->min_pixels >= 6;
}

// What does not need the map, first, so that nothing of a wrong call reaches a handle.  Not the fuse's check (voxel_host.hip): an
// alignment weighs a row by f base / Z^2, so f and base must be positive as well as finite; its int64 sums of up to two products
// below 2^40 a pixel stay below 2^63 for at most 2^22 pixels, a limit of the definition (include/viso_hip.h), so a larger map is
// a wrong argument, not an unsupported one.
static int align_check(const char* where, const viso_tsdf_align_params* p, const DispView& v) {
    if (!align_params_ok(p)) {
        viso_set_error("%s: bad argument (parameters: min_weight >= 1, a finite gate_voxels > 0, max_iters in 1..50, finite eps_rot and "
                       "eps_trans >= 0, min_pixels >= 6)", where);
        return VISO_ERR_ARG;
    }
    if (v.rows < 1 || v.cols < 1 || (long long)v.rows * v.cols > ALIGN_MAX_PIXELS) {
        viso_set_error("%s: bad argument (a %d x %d map: sizes >= 1 and at most 2^22 pixels)", where, v.rows, v.cols);
        return VISO_ERR_ARG;
    }
    const StereoCalib& c = v.cal;
    if (!(std::isfinite(c.f) && std::isfinite(c.cu) && std::isfinite(c.cv) && std::isfinite(c.base) && c.f > 0.0 && c.base > 0.0)) {
        viso_set_error("%s: bad argument (the calibration f, cu, cv, base must be finite, f > 0 and base > 0)", where);
        return VISO_ERR_ARG;
    }
    if (v.poses) {
        for (int k = 0; k < v.n; ++k) {
            for (int i = 0; i < 12; ++i) {
                if (!std::isfinite(v.poses[(size_t)k * 16 + i])) { viso_set_error("%s: bad argument (pose %d has an entry that is not finite)", where, k); return VISO_ERR_ARG; }
            }
        }
    }
    return VISO_OK;
}

// What does not need the map, for the photometric alignment: the image, the photometric parameters, then align_check.
static int align_gray_check(const char* where, const viso_tsdf_align_gray_params* p, const DispView& v) {
    if (!p || !v.image) { viso_set_error("%s: bad argument (non-null parameters and image)", where); return VISO_ERR_ARG; }
    if (!(std::isfinite(p->photo_weight) && p->photo_weight >= 0.0 && std::isfinite(p->photo_gate) && p->photo_gate > 0.0)) {
        viso_set_error("%s: bad argument (parameters: a finite photo_weight >= 0 and a finite photo_gate > 0)", where);
        return VISO_ERR_ARG;
    }
    return align_check(where, &p->geo, v);
}

void AlignPlain::launch(const TsdfAlignArgs& g, dim3 grid, hipStream_t s) { hipLaunchKernelGGL(tsdf_linearize_kernel, grid, dim3(256), 0, s, g); }
void AlignGray::launch(const TsdfGrayAlignArgs& g, dim3 grid, hipStream_t s) { hipLaunchKernelGGL(tsdf_gray_linearize_kernel, grid, dim3(256), 0, s, g); }
static TsdfAlignArgs& align_geo_args(TsdfAlignArgs& g) { return g; }
static TsdfAlignArgs& align_geo_args(TsdfGrayAlignArgs& g) { return g.a; }

// One call of kind K (alignmath.h): the maps, the parameters, and where the result goes.  linearize_out set: one linearise at the
// view's poses and nothing else; otherwise one record a frame and, for frame 0, at most trace_cap entries of trace (or null).
template <class K>
struct AlignRequest {
    DispView v;
    const typename K::Params* p;
    typename K::Normal* linearize_out;
    typename K::Record* records; typename K::Step* trace; int trace_cap;
};

// The alignment of a view's maps behind align_check: the handle entered and locked like an extraction over all of its linearises.
// A resident view's context must be the map's; a host view's map (and image) goes through the fuse's staging.  AlignGray: the
// photometric alignment of a gray map.
template <class K>
static int align_device(const char* where, viso_tsdf* t, const AlignRequest<K>& q) {
    constexpr bool photo = K::words == ALIGN_GRAY_WORDS;
    static_assert(AlignPlain::words == ALIGN_WORDS && AlignGray::words == ALIGN_GRAY_WORDS, "the kernels' words are the structs");
    const DispView& v = q.v;
    const viso_tsdf_align_params& p = K::geo(*q.p);
    VoxelRegistry& reg = tsdf_registry();
    if (!voxel_known(reg, t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    if (photo && !tsdf_is_gray(t)) {   // before a device is touched
        viso_set_error("%s: the TSDF map carries no intensity (viso_tsdf_create_gray makes one that does)", where);
        return VISO_ERR_ARG;
    }
    VoxelSession ses(where, reg, t, VoxelSession::ANY_STATE);   // the overflow refusal comes behind the two checks that need the map
    VISO_TRY(ses.status());
    VoxelHost* h = ses.host();
    if (v.ctx && h->ctx != v.ctx) { viso_set_error("%s: the TSDF map and the batch must share a context", where); return VISO_ERR_ARG; }
    TsdfView view;
    tsdf_view(t, &view);
    if (p.gate_voxels > (double)view.trunc_voxels) {
        viso_set_error("%s: bad argument (gate_voxels %g is beyond the map's truncation of %d voxels)", where, p.gate_voxels, view.trunc_voxels);
        return VISO_ERR_ARG;
    }
    VISO_TRY(ses.refuse_overflowed());
    const size_t px = v.px();
    const int16_t* disp = v.disp;
    const uint8_t* image = v.image;
    if (!v.ctx) {
        VISO_TRY(voxel_stage_map(where, h, v.disp, px, &disp));
        if (v.image) VISO_TRY(voxel_stage_image(where, h, v.image, px, &image));
    }
    TsdfAlignArgs a;
    a.v.mfs = v.mfs; a.v.rows = v.rows; a.v.cols = v.cols; a.v.min_disp16 = h->min_disp16; a.v._pad = 0;
    a.v.f = v.cal.f; a.v.cu = v.cal.cu; a.v.cv = v.cal.cv; a.v.base = v.cal.base;
    a.t = view.t;
    a.voxel = view.voxel; a.s = view.s; a.gate = p.gate_voxels * 1024.0; a.min_weight = p.min_weight;
    const size_t blocks = (px + 255) / 256;
    const unsigned blocks_x = blocks < ALIGN_BLOCKS ? (unsigned)blocks : ALIGN_BLOCKS;
    a.trips = (int)((px + (size_t)blocks_x * 256 - 1) / ((size_t)blocks_x * 256));
    const AlignLinearize<K> linearize = [&](const double* poses, const unsigned long long* active, typename K::Normal* out) {
        return voxel_linearize(where, h, poses, active, v.n, K::words, reinterpret_cast<unsigned long long*>(out),
                               [&](const double* d_poses, const unsigned long long* d_active, unsigned long long* d_out, int frame0, unsigned frames, hipStream_t st) {
            typename K::Args g;
            TsdfAlignArgs& ga = align_geo_args(g);
            ga = a;
            ga.v.disp = disp + (size_t)frame0 * v.mfs; ga.v.poses = d_poses; ga.active = d_active; ga.out = d_out;
            if constexpr (photo) {
                g.gray = view.gray; g.image = image + (size_t)frame0 * v.ifs; g.ifs = v.ifs;
                g.lambda = q.p->photo_weight; g.photo_gate = q.p->photo_gate;
            }
            K::launch(g, dim3(blocks_x, frames), st);
        });
    };
    static const double eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const unsigned long long one = 1ull;
    if (q.linearize_out) return linearize(v.poses ? v.poses : eye, &one, q.linearize_out);
    return align_run<K>(*q.p, v.n, v.poses, linearize, q.records, q.trace, q.trace_cap);
}

extern "C" int viso_tsdf_linearize(viso_tsdf* t, const viso_tsdf_align_params* params, const int16_t* disp, int rows, int cols,
                                   const viso_param* param, const double* pose_or_null, viso_tsdf_normal* out) {
    const char* where = "viso_tsdf_linearize";
    if (!disp || !param || !out) { viso_set_error("%s: bad argument (non-null map, calibration and output)", where); return VISO_ERR_ARG; }
    const DispView v = disp_view_host(disp, nullptr, rows, cols, param, pose_or_null);
    VISO_TRY(align_check(where, params, v));
    return align_device<AlignPlain>(where, t, {v, params, out, nullptr, nullptr, 0});
}

extern "C" int viso_tsdf_align(viso_tsdf* t, const viso_tsdf_align_params* params, const int16_t* disp, int rows, int cols, const viso_param* param,
                               const double* pose_guess_or_null, viso_tsdf_alignment* record_out, viso_tsdf_align_step* trace_out_or_null,
                               int trace_cap) {
    const char* where = "viso_tsdf_align";
    if (!disp || !param || !record_out || trace_cap < 0 || (trace_cap && !trace_out_or_null)) {
        viso_set_error("%s: bad argument (non-null map, calibration and record, trace_cap >= 0 and 0 without a trace)", where);
        return VISO_ERR_ARG;
    }
    const DispView v = disp_view_host(disp, nullptr, rows, cols, param, pose_guess_or_null);
    VISO_TRY(align_check(where, params, v));
    return align_device<AlignPlain>(where, t, {v, params, nullptr, record_out, trace_out_or_null, trace_cap});
}

int tsdf_align_resident(const char* where, viso_tsdf* t, const DispView& v, const viso_tsdf_align_params* params, viso_tsdf_alignment* records) {
    VISO_TRY(align_check(where, params, v));
    return align_device<AlignPlain>(where, t, {v, params, nullptr, records, nullptr, 0});
}

// ---- the photometric alignment (include/viso_hip.h, "TSDF photometric align") ----------------------------------------------------------
extern "C" void viso_tsdf_align_gray_params_default(viso_tsdf_align_gray_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    viso_tsdf_align_params_default(&p->geo);
    p->photo_weight = 1.0 / 32.0; p->photo_gate = 255.0;
}

extern "C" int viso_tsdf_linearize_gray(viso_tsdf* t, const viso_tsdf_align_gray_params* params, const int16_t* disp, const uint8_t* image, int rows,
                                        int cols, const viso_param* param, const double* pose_or_null, viso_tsdf_normal_gray* out) {
    const char* where = "viso_tsdf_linearize_gray";
    if (!disp || !param || !out) { viso_set_error("%s: bad argument (non-null map, calibration and output)", where); return VISO_ERR_ARG; }
    const DispView v = disp_view_host(disp, image, rows, cols, param, pose_or_null);
    VISO_TRY(align_gray_check(where, params, v));
    return align_device<AlignGray>(where, t, {v, params, out, nullptr, nullptr, 0});
}

extern "C" int viso_tsdf_align_gray(viso_tsdf* t, const viso_tsdf_align_gray_params* params, const int16_t* disp, const uint8_t* image, int rows,
                                    int cols, const viso_param* param, const double* pose_guess_or_null, viso_tsdf_alignment_gray* record_out,
                                    viso_tsdf_align_gray_step* trace_out_or_null, int trace_cap) {
    const char* where = "viso_tsdf_align_gray";
    if (!disp || !param || !record_out || trace_cap < 0 || (trace_cap && !trace_out_or_null)) {
        viso_set_error("%s: bad argument (non-null map, calibration and record, trace_cap >= 0 and 0 without a trace)", where);
        return VISO_ERR_ARG;
    }
    const DispView v = disp_view_host(disp, image, rows, cols, param, pose_guess_or_null);
    VISO_TRY(align_gray_check(where, params, v));
    return align_device<AlignGray>(where, t, {v, params, nullptr, record_out, trace_out_or_null, trace_cap});
}

int tsdf_align_gray_resident(const char* where, viso_tsdf* t, const DispView& v, const viso_tsdf_align_gray_params* params,
                             viso_tsdf_alignment_gray* records) {
    VISO_TRY(align_gray_check(where, params, v));
    return align_device<AlignGray>(where, t, {v, params, nullptr, records, nullptr, 0});
}
