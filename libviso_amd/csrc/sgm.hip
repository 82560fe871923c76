// sgm.hip — opt-in semi-global matching of rectified pairs (NOT in the reference: viso_stereo_sgm, viso_batch_set_sgm,
// include/viso_hip.h).  Census 9 x 7, Hamming cost, 4 or 8 paths with penalties P1 / P2, then the selection of the
// block matcher (disparity.hip) on the summed costs.  Everything is an exact integer: the device output is bit-identical to
// tests/sgm_ref.py.
//
// Per group of frames (as many as the workspace holds):
//   sgm_census_kernel   one thread per pixel and side: the 62-bit census word                        -> cen [frame][2][rows][cols] u64
//   sgm_path_kernel     once per direction r.  One wave per path LINE, lanes over d (K = ceil(D / 64) consecutive disparities per
//                       lane), walking the line pixel by pixel with L_r(p - r, .) in registers.  A line of a horizontal path is a
//                       row; a line of a vertical or diagonal path starts at column c of the first row and moves by dx per row,
//                       wrapping at the image's side: where it wraps, p - r is outside the image and the path starts again, so the
//                       lines of one direction partition the pixels and no state crosses waves.  The cost is recomputed from the
//                       census words at every step (two v_bcnt_u32_b32 per disparity), the minimum over d is six DPP steps and a
//                       v_readlane, the d +- 1 neighbours are wave shifts.  S [frame][rows][cols][D] u16 is written by the first
//                       direction and added to by the others: every element has one owner per launch, launches are ordered by the
//                       stream, so there are no atomics and no dependence on scheduling.
//   sgm_select_kernel   one workgroup per row: the right pixels' keys min((S(xr + d, d) << 8) | d) into LDS, then every left
//                       pixel's sweep over d with the block matcher's running state (S*, d*, the two neighbours, the best cost
//                       before d* - 1 and after d* + 1), uniqueness, left-right check, V-fit                -> out i16
// L_r <= 62 + P2 <= 254, S <= 8 * 254 = 2032.
#include "common.h"
#include "wave.h"

#define SGM_MAX_COLS 2048
#define SGM_SEL_THREADS 256
#define SGM_BIG 0x3fffu           // a disparity that is not a candidate (P1, P2 <= 192 can be added without overflow)
#define SGM_DEFAULT_CAP ((size_t)2 << 30)

// ---- census --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sgm_census_kernel(const uint8_t* __restrict__ img, size_t fs, size_t ss, int rows, int cols,
                                                         unsigned long long* __restrict__ cen, size_t cfs) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, f = blockIdx.z >> 1, side = blockIdx.z & 1;
    if (x >= cols) return;
    const uint8_t* I = img + (size_t)f * fs + (size_t)side * ss;
    const uint32_t c = I[(size_t)y * cols + x];
    unsigned long long w = 0;
    int bit = 0;
#pragma unroll
    for (int j = -3; j <= 3; ++j) {
        const uint8_t* row = I + (size_t)min(max(y + j, 0), rows - 1) * cols;
#pragma unroll
        for (int i = -4; i <= 4; ++i) {
            if (i == 0 && j == 0) continue;
            const uint32_t v = row[min(max(x + i, 0), cols - 1)];
            w |= (unsigned long long)(v < c ? 1u : 0u) << bit;
            ++bit;
        }
    }
    cen[(size_t)f * cfs + ((size_t)side * rows + y) * cols + x] = w;
}

// ---- one path direction ----------------------------------------------------------------------------------------------------
struct SgmPathArgs {
    const unsigned long long* cen; size_t cfs;   // frame f's words at cen + f * cfs: left [rows][cols], then right
    uint16_t* S; size_t sfs;                     // frame f's sums at S + f * sfs
    int rows, cols, D, P1, P2;
    int dx, dy;                                  // the direction r
    int first;                                   // 1: S = L_r (the first direction); 0: S += L_r
};

template <int K>
__global__ __launch_bounds__(64) void sgm_path_kernel(SgmPathArgs a) {
    const int lane = threadIdx.x, line = blockIdx.x, f = blockIdx.y;
    const int rows = a.rows, cols = a.cols, D = a.D, dx = a.dx, dy = a.dy;
    const unsigned long long* cL = a.cen + (size_t)f * a.cfs;
    const unsigned long long* cR = cL + (size_t)rows * cols;
    uint16_t* S = a.S + (size_t)f * a.sfs;
    const uint32_t P1 = (uint32_t)a.P1, P2 = (uint32_t)a.P2;
    const int d0 = lane * K;                     // this lane's disparities d0 .. d0 + K - 1
    const int steps = dy == 0 ? cols : rows;
    uint32_t prev[K];
#pragma unroll
    for (int k = 0; k < K; ++k) prev[k] = SGM_BIG;
    int x = dy == 0 ? (dx > 0 ? 0 : cols - 1) : line;
    int y = dy == 0 ? line : (dy > 0 ? 0 : rows - 1);
    for (int s = 0; s < steps; ++s) {
        const int xp = x - dx;
        const bool start = s == 0 || xp < 0 || xp >= cols;       // p - r is outside the image: the path starts here
        const size_t pix = (size_t)y * cols + x;
        const unsigned long long wl = cL[pix];
        const int dcap = min(D - 1, x);                          // candidates of p: d <= dcap
        uint32_t C[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int d = d0 + k;
            C[k] = d <= dcap ? (uint32_t)__popcll(wl ^ cR[pix - d]) : SGM_BIG;
        }
        // M and the neighbours: computed by every lane, outside any divergent branch (the DPP steps need the whole wave)
        uint32_t mn = prev[0];
#pragma unroll
        for (int k = 1; k < K; ++k) mn = min(mn, prev[k]);
        const uint32_t M = (uint32_t)__builtin_amdgcn_readlane((int)viso_wave_min63(mn), 63);
        const uint32_t below = viso_dpp<0x138, 0xf>(prev[K - 1], SGM_BIG);   // wave_shr:1: the lane before's last disparity
        const uint32_t above = viso_dpp<0x130, 0xf>(prev[0], SGM_BIG);       // wave_shl:1: the lane after's first one
        uint32_t cur[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t lo = k > 0 ? prev[k - 1] : below;
            const uint32_t hi = k < K - 1 ? prev[k + 1] : above;
            const uint32_t t = min(min(prev[k], M + P2), min(lo, hi) + P1);
            cur[k] = C[k] >= SGM_BIG ? SGM_BIG : (start ? C[k] : C[k] + t - M);
        }
        // S of the candidates (0 where d is not one: the selection never reads those)
        if (d0 < D) {
            uint16_t* sp = S + pix * (size_t)D + d0;
            if constexpr (K == 2) {
                uint32_t v = a.first ? 0u : *reinterpret_cast<const uint32_t*>(sp);
                const uint32_t l0 = cur[0] >= SGM_BIG ? 0u : cur[0], l1 = cur[1] >= SGM_BIG ? 0u : cur[1];
                v += l0 | (l1 << 16);                            // sums <= 2032: no carry between the halves
                *reinterpret_cast<uint32_t*>(sp) = v;
            } else if constexpr (K == 4) {
                uint2 v = a.first ? make_uint2(0u, 0u) : *reinterpret_cast<const uint2*>(sp);
                const uint32_t l0 = cur[0] >= SGM_BIG ? 0u : cur[0], l1 = cur[1] >= SGM_BIG ? 0u : cur[1];
                const uint32_t l2 = cur[2] >= SGM_BIG ? 0u : cur[2], l3 = cur[3] >= SGM_BIG ? 0u : cur[3];
                v.x += l0 | (l1 << 16); v.y += l2 | (l3 << 16);
                *reinterpret_cast<uint2*>(sp) = v;
            } else {
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (d0 + k < D) {
                        const uint32_t l = cur[k] >= SGM_BIG ? 0u : cur[k];
                        sp[k] = (uint16_t)((a.first ? 0u : (uint32_t)sp[k]) + l);
                    }
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) prev[k] = cur[k];
        if (dy == 0) x += dx;
        else {
            y += dy;
            x += dx;
            x = x < 0 ? cols - 1 : (x >= cols ? 0 : x);
        }
    }
}

// ---- selection -------------------------------------------------------------------------------------------------------------
struct SgmSelArgs {
    const uint16_t* S; size_t sfs;
    int16_t* out; size_t ofs;
    int rows, cols, D, u, m;
};

__global__ __launch_bounds__(SGM_SEL_THREADS) void sgm_select_kernel(SgmSelArgs a) {
    __shared__ uint8_t dR[SGM_MAX_COLS];
    const int y = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const int cols = a.cols, D = a.D;
    const uint16_t* S = a.S + (size_t)f * a.sfs + (size_t)y * cols * D;
    int16_t* out = a.out + (size_t)f * a.ofs + (size_t)y * cols;
    if (a.m >= 0) {
        // the right pixels: the diagonal (xr + d, d) of the row's sums
        for (int xr = tid; xr < cols; xr += SGM_SEL_THREADS) {
            const int dl = min(D - 1, cols - 1 - xr);
            uint32_t key = 0xffffffffu;
            const uint16_t* p = S + (size_t)xr * D;
            for (int d = 0; d <= dl; ++d) key = min(key, ((uint32_t)p[(size_t)d * (D + 1)] << 8) | (uint32_t)d);
            dR[xr] = (uint8_t)(key & 0xffu);
        }
        __syncthreads();
    }
    for (int x = tid; x < cols; x += SGM_SEL_THREADS) {
        const int dmax = min(D - 1, x);
        const uint4* p = reinterpret_cast<const uint4*>(S + (size_t)x * D);   // D is a multiple of 16: 32-byte aligned
        // d ascending: the first strict minimum is the smallest d among equal sums
        uint32_t Sb = 0xffffffffu, ds = 0, cn = 0, cp = 0, pre_best = 0xffffffffu, outm = 0xffffffffu, pre = 0xffffffffu,
                 c1 = 0xffffffffu, c2 = 0xffffffffu;
        for (int d8 = 0; d8 <= dmax; d8 += 8) {
            const uint4 q = p[d8 >> 3];
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int d = d8 + e;
                if (d <= dmax) {
                    const uint32_t v = (w[e >> 1] >> (16 * (e & 1))) & 0xffffu;
                    pre = min(pre, c2);                        // min of S(0 .. d-2)
                    if (v < Sb) {                              // a new best: d* = d
                        pre_best = pre; cn = c1; cp = 0xffffffffu; outm = 0xffffffffu;
                        Sb = v; ds = (uint32_t)d;
                    } else if ((uint32_t)d == ds + 1) {
                        cp = v;
                    } else {
                        outm = min(outm, v);                   // d >= d* + 2
                    }
                    c2 = c1; c1 = v;
                }
            }
        }
        bool ok = true;
        if (a.u > 0) {
            const uint32_t thr = Sb + (Sb * (uint32_t)a.u) / 100u;
            ok = min(pre_best, outm) > thr;
        }
        if (ok && a.m >= 0) ok = abs((int)dR[x - (int)ds] - (int)ds) <= a.m;
        int v = VISO_DISP_INVALID;
        if (ok) {
            int off = 0;
            if (ds > 0 && (int)ds < dmax) {
                const int pp = (int)cp, nn = (int)cn;
                const int k = pp + nn - 2 * (int)Sb + abs(pp - nn);
                off = k ? ((nn - pp) * 256) / k : 0;
            }
            v = (256 * (int)ds + off + 8) >> 4;
        }
        out[x] = (int16_t)v;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
bool sgm_params_ok(const viso_sgm_params* p) {
    return p && p->num_disp >= 16 && p->num_disp <= 256 && p->num_disp % 16 == 0 && p->p1 >= 1 && p->p1 <= p->p2 && p->p2 <= 192 &&
           (p->paths == 4 || p->paths == 8) && p->uniqueness >= 0 && p->uniqueness <= 100 && p->lr_max_diff >= -1 &&
           p->lr_max_diff <= p->num_disp;
}

bool sgm_geometry_ok(int rows, int cols) { return rows > 0 && cols > 0 && cols <= SGM_MAX_COLS; }

extern "C" void viso_sgm_params_default(viso_sgm_params* p) {
    if (!p) return;
    p->num_disp = 128; p->p1 = 10; p->p2 = 120; p->paths = 8; p->uniqueness = 10; p->lr_max_diff = 1;
}

static WorkspaceCap g_sgm_cap{{SGM_DEFAULT_CAP}, SGM_DEFAULT_CAP, "SGM", "viso_sgm_set_workspace_cap"};

extern "C" void viso_sgm_set_workspace_cap(size_t bytes) { g_sgm_cap.set(bytes); }

size_t sgm_frame_bytes(int rows, int cols, int D) {
    const size_t px = (size_t)rows * cols;
    return al256(px * 2 * sizeof(unsigned long long)) + al256(px * (size_t)D * sizeof(uint16_t));
}

int sgm_group_frames(const char* where, int rows, int cols, int D, int n_frames, int* group) {
    return g_sgm_cap.frames(where, rows, cols, sgm_frame_bytes(rows, cols, D), n_frames, 16384, group);   // 2 * group workgroups along the census grid's z
}

int launch_sgm(hipStream_t s, const StereoImages& im, const viso_sgm_params* p, int16_t* out, size_t ofs, void* ws, int group) {
    if (im.n <= 0) return VISO_OK;
    const int D = p->num_disp;
    const size_t px = im.px();
    const size_t cen_bytes = al256(px * 2 * sizeof(unsigned long long));
    const size_t per = sgm_frame_bytes(im.rows, im.cols, D);
    static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
    const int K = (D + 63) / 64;
    for (int f0 = 0; f0 < im.n; f0 += group) {
        const int nf = im.n - f0 < group ? im.n - f0 : group;
        unsigned long long* cen = reinterpret_cast<unsigned long long*>(ws);
        uint16_t* S = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(ws) + cen_bytes);
        const uint8_t* img = im.img + (size_t)f0 * im.fs;
        hipLaunchKernelGGL(sgm_census_kernel, dim3((unsigned)((im.cols + 255) / 256), (unsigned)im.rows, (unsigned)(2 * nf)), dim3(256), 0, s,
                           img, im.fs, im.ss, im.rows, im.cols, cen, per / sizeof(unsigned long long));
        SgmPathArgs a;
        a.cen = cen; a.cfs = per / sizeof(unsigned long long); a.S = S; a.sfs = per / sizeof(uint16_t);
        a.rows = im.rows; a.cols = im.cols; a.D = D; a.P1 = p->p1; a.P2 = p->p2;
        for (int r = 0; r < p->paths; ++r) {
            a.dx = dirs[r][0]; a.dy = dirs[r][1]; a.first = r == 0;
            const dim3 grid((unsigned)(a.dy == 0 ? im.rows : im.cols), (unsigned)nf);
            switch (K) {
                case 1: hipLaunchKernelGGL(sgm_path_kernel<1>, grid, dim3(64), 0, s, a); break;
                case 2: hipLaunchKernelGGL(sgm_path_kernel<2>, grid, dim3(64), 0, s, a); break;
                case 3: hipLaunchKernelGGL(sgm_path_kernel<3>, grid, dim3(64), 0, s, a); break;
                default: hipLaunchKernelGGL(sgm_path_kernel<4>, grid, dim3(64), 0, s, a); break;
            }
        }
        SgmSelArgs e;
        e.S = S; e.sfs = per / sizeof(uint16_t); e.out = out + (size_t)f0 * ofs; e.ofs = ofs;
        e.rows = im.rows; e.cols = im.cols; e.D = D; e.u = p->uniqueness; e.m = p->lr_max_diff;
        hipLaunchKernelGGL(sgm_select_kernel, dim3((unsigned)im.rows, (unsigned)nf), dim3(SGM_SEL_THREADS), 0, s, e);
        HIP_TRY(hipGetLastError());
    }
    return VISO_OK;
}

// One pair of host images on the default context.
extern "C" int viso_stereo_sgm(const uint8_t* left, const uint8_t* right, int rows, int cols, const viso_sgm_params* params,
                               int16_t* out) {
    if (!left || !right || !out || rows <= 0 || cols <= 0 || !sgm_params_ok(params)) {
        viso_set_error("viso_stereo_sgm: bad argument (non-null images and output, sizes > 0, parameters of include/viso_hip.h)");
        return VISO_ERR_ARG;
    }
    if (!sgm_geometry_ok(rows, cols)) {
        viso_set_error("viso_stereo_sgm: %d columns exceed the %d this build handles", cols, SGM_MAX_COLS);
        return VISO_ERR_UNSUPPORTED;
    }
    VISO_TRY(sgm_group_frames("viso_stereo_sgm", rows, cols, params->num_disp, 1, nullptr));
    const size_t per = (size_t)rows * cols;
    DirectCall dc;
    VISO_TRY(dc.begin());
    uint8_t* dimg; int16_t* dout; char* ws;
    VISO_TRY(dc.scratch(SLOT_GEN0, 2 * per, &dimg));
    VISO_TRY(dc.scratch(SLOT_GEN1, per, &dout));
    VISO_TRY(dc.scratch(SLOT_GEN2, sgm_frame_bytes(rows, cols, params->num_disp), &ws));
    VISO_TRY(dc.up(dimg, left, per));
    VISO_TRY(dc.up(dimg + per, right, per));
    VISO_TRY(launch_sgm(dc.s, image_block(dimg, rows, cols, 0, 1), params, dout, per, ws, 1));
    VISO_TRY(dc.down(out, dout, per));
    return dc.wait();
}
