// disparity.hip — opt-in dense stereo disparity of rectified pairs (NOT in the reference: viso_stereo_disparity,
// viso_batch_set_disparity, include/viso_hip.h).  The definition is StereoBM's: XSOBEL prefilter clamped to
// [-c, c] and shifted by c, SAD block of B x B, texture threshold, uniqueness ratio, a 1/16-px V-fit and an order-free
// left-right check.  Everything is an exact integer: the device output is bit-identical to tests/disparity_ref.py.
//
// One workgroup per (inside row, frame), all columns of the row (cols <= DISP_MAX_COLS).  The row's prefiltered windows are
// staged in LDS once as packed columns: dword k of column x holds P(x, y - r + 4k + b) in byte b (rows past the block are 0 in
// both images), so the vertical SAD of a column at one disparity is ceil(B / 4) v_sad_u8.  Then one step per disparity d:
//   A  every column's vertical SAD  V(x, d) = sum_j |P_L(x, y+j) - P_R(x-d, y+j)|          -> LDS row
//   B  every pixel's cost C(x, d) = sum_i V(x+i, d), a running sum along the thread's run of columns; the per-pixel state
//      (best cost and disparity, its neighbours' costs, the smallest cost outside d* +- 1) is updated in registers -> LDS row
//   C  every right pixel xr's key min((C(xr+d, d) << 8) | d): the diagonal of the cost volume, read from the same LDS row
// The cost volume never leaves the workgroup.  Costs are at most 2c B^2 = 55 566 < 2^16, so the keys fit 24 bits.
#include "common.h"

#include <vector>

#define DISP_THREADS 256
#define DISP_RUN 8                                   // columns per thread at most
#define DISP_MAX_COLS (DISP_THREADS * DISP_RUN)      // 2048
#define DISP_INF 0x7fffffffu

__device__ __forceinline__ int disp_reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

// P(x, y) of one image: the extractor's Sobel-x (3x3, BORDER_REFLECT_101 on both axes), clamped to [-c, c], plus c.
__device__ __forceinline__ uint32_t disp_prefilter(const uint8_t* __restrict__ img, int rows, int cols, int x, int y, int c) {
    const uint8_t* r0 = img + (size_t)disp_reflect101(y - 1, rows) * cols;
    const uint8_t* r1 = img + (size_t)y * cols;
    const uint8_t* r2 = img + (size_t)disp_reflect101(y + 1, rows) * cols;
    const int xm = disp_reflect101(x - 1, cols), xp = disp_reflect101(x + 1, cols);
    const int g = ((int)r0[xp] - (int)r0[xm]) + 2 * ((int)r1[xp] - (int)r1[xm]) + ((int)r2[xp] - (int)r2[xm]);
    return (uint32_t)(min(max(g, -c), c) + c);
}

struct DispArgs {
    const uint8_t* img; size_t fs, ss;   // left image of frame f at img + f * fs, right at + ss
    int16_t* out; size_t ofs;            // frame f's map at out + f * ofs
    int rows, cols;
    viso_disparity_params p;
};

// Rows that are not inside are written by the same kernel (blockIdx.x covers every row): all VISO_DISP_INVALID.
__global__ __launch_bounds__(DISP_THREADS) void stereo_disparity_kernel(DispArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t d_smem[];
    const int y = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const int rows = a.rows, cols = a.cols;
    const int D = a.p.num_disp, B = a.p.block, c = a.p.prefilter_cap, r = B / 2;
    const int K = (B + 3) / 4;
    int16_t* out = a.out + (size_t)f * a.ofs + (size_t)y * cols;
    const int run = (cols + DISP_THREADS - 1) / DISP_THREADS;   // <= DISP_RUN
    const int x0 = tid * run;
    if (y < r || y >= rows - r || cols < B) {
        for (int x = tid; x < cols; x += DISP_THREADS) out[x] = (int16_t)VISO_DISP_INVALID;
        return;
    }
    const uint8_t* L = a.img + (size_t)f * a.fs;
    const uint8_t* R = L + a.ss;
    uint32_t* PL = d_smem;                 // [K][cols]
    uint32_t* PR = PL + (size_t)K * cols;  // [K][cols]
    uint32_t* V = PR + (size_t)K * cols;   // [cols]: vertical SADs, then the texture column sums, then dR
    uint32_t* CS = V + cols;               // [cols]: the costs of the current disparity

    // the packed columns of the row's window
    for (int e = tid; e < K * cols; e += DISP_THREADS) {
        const int k = e / cols, x = e - k * cols;
        uint32_t wl = 0, wr = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = 4 * k + b;
            if (j < B) {
                wl |= disp_prefilter(L, rows, cols, x, y - r + j, c) << (8 * b);
                wr |= disp_prefilter(R, rows, cols, x, y - r + j, c) << (8 * b);
            }
        }
        PL[e] = wl; PR[e] = wr;
    }
    __syncthreads();

    // texture: sum over the window of |P_L - c|; the 4K - B padding bytes (0) each add c
    const uint32_t cc = (uint32_t)c * 0x01010101u, pad = (uint32_t)(4 * K - B) * (uint32_t)c;
    for (int x = tid; x < cols; x += DISP_THREADS) {
        uint32_t s = 0;
        for (int k = 0; k < K; ++k) s = __builtin_amdgcn_sad_u8(PL[k * cols + x], cc, s);
        V[x] = s - pad;
    }
    __syncthreads();
    // this thread's pixels: x0 + i, i < run; inside columns are r <= x < cols - r
    const int xa = max(x0, r), xb = min(x0 + run, cols - r);   // the thread's inside pixels [xa, xb)
    bool tex_ok[DISP_RUN];
    {
        uint32_t s = 0;
        if (xa < xb)
            for (int i = -r; i <= r; ++i) s += V[xa + i];
#pragma unroll
        for (int i = 0; i < DISP_RUN; ++i) {
            const int x = x0 + i;
            tex_ok[i] = true;
            if (x >= xa && x < xb) {
                if (x > xa) s += V[x + r] - V[x - r - 1];
                tex_ok[i] = (long long)s >= (long long)a.p.texture_threshold;
            }
        }
    }
    __syncthreads();

    // per-pixel state of the disparity sweep (d ascending: the first strict minimum is the smallest d among equal costs)
    uint32_t S[DISP_RUN], dst[DISP_RUN], cn[DISP_RUN], cp[DISP_RUN], pre_best[DISP_RUN], outm[DISP_RUN], pre[DISP_RUN],
        c1[DISP_RUN], c2[DISP_RUN], keyR[DISP_RUN];
#pragma unroll
    for (int i = 0; i < DISP_RUN; ++i) {
        S[i] = DISP_INF; dst[i] = 0; cn[i] = DISP_INF; cp[i] = DISP_INF; pre_best[i] = DISP_INF; outm[i] = DISP_INF;
        pre[i] = DISP_INF; c1[i] = DISP_INF; c2[i] = DISP_INF; keyR[i] = DISP_INF;
    }
    const int dlim = min(D - 1, cols - 1 - 2 * r);   // the largest candidate of any inside pixel
    for (int d = 0; d <= dlim; ++d) {
        // A: vertical SADs of the columns x >= d (the only ones a candidate's window reads)
#pragma unroll
        for (int i = 0; i < DISP_RUN; ++i) {
            const int x = x0 + i;
            if (i < run && x < cols && x >= d) {
                uint32_t s = 0;
                for (int k = 0; k < K; ++k) s = __builtin_amdgcn_sad_u8(PL[k * cols + x], PR[k * cols + x - d], s);
                V[x] = s;
            }
        }
        __syncthreads();
        // B: costs of the thread's inside pixels with d <= dmax(x) = min(D - 1, x - r), i.e. x >= d + r
        const int xs = max(xa, d + r);
        uint32_t s = 0;
        if (xs < xb)
            for (int i = -r; i <= r; ++i) s += V[xs + i];
#pragma unroll
        for (int i = 0; i < DISP_RUN; ++i) {
            const int x = x0 + i;
            if (x >= xs && x < xb) {
                if (x > xs) s += V[x + r] - V[x - r - 1];
                const uint32_t C = s;
                CS[x] = C;
                const uint32_t p2 = c2[i];
                pre[i] = min(pre[i], p2);                  // min of C(0 .. d-2)
                if (C < S[i]) {                            // a new best: d* = d
                    pre_best[i] = pre[i]; cn[i] = c1[i]; cp[i] = DISP_INF; outm[i] = DISP_INF;
                    S[i] = C; dst[i] = (uint32_t)d;
                } else if ((uint32_t)d == dst[i] + 1) {
                    cp[i] = C;
                } else {
                    outm[i] = min(outm[i], C);             // d >= d* + 2
                }
                c2[i] = c1[i]; c1[i] = C;
            }
        }
        __syncthreads();
        // C: right pixels xr >= r whose left partner xr + d is an inside pixel
#pragma unroll
        for (int i = 0; i < DISP_RUN; ++i) {
            const int xr = x0 + i;
            if (i < run && xr >= r && xr + d < cols - r) keyR[i] = min(keyR[i], (CS[xr + d] << 8) | (uint32_t)d);
        }
    }
    __syncthreads();   // every step's reads of V and CS are done: V now carries dR
#pragma unroll
    for (int i = 0; i < DISP_RUN; ++i) {
        const int xr = x0 + i;
        if (i < run && xr < cols) V[xr] = keyR[i] & 0xffu;
    }
    __syncthreads();
    const int u = a.p.uniqueness, m = a.p.lr_max_diff;
#pragma unroll
    for (int i = 0; i < DISP_RUN; ++i) {
        const int x = x0 + i;
        if (i >= run || x >= cols) continue;
        int v = VISO_DISP_INVALID;
        if (x >= xa && x < xb && tex_ok[i]) {
            const int ds = (int)dst[i], dmax = min(D - 1, x - r);
            const int Sb = (int)S[i];
            bool ok = true;
            if (u > 0) {
                const uint32_t thr = S[i] + (S[i] * (uint32_t)u) / 100u;
                ok = min(pre_best[i], outm[i]) > thr;
            }
            if (ok && m >= 0) {
                const int dr = (int)V[x - ds];
                ok = abs(dr - ds) <= m;
            }
            if (ok) {
                int off = 0;
                if (ds > 0 && ds < dmax) {
                    const int pp = (int)cp[i], nn = (int)cn[i];
                    const int k = pp + nn - 2 * Sb + abs(pp - nn);
                    off = k ? ((nn - pp) * 256) / k : 0;
                }
                v = (256 * ds + off + 8) >> 4;
            }
        }
        out[x] = (int16_t)v;
    }
}

bool disparity_params_ok(const viso_disparity_params* p) {
    return p && p->num_disp >= 16 && p->num_disp <= 256 && p->num_disp % 16 == 0 && p->block >= 5 && p->block <= 21 &&
           p->block % 2 == 1 && p->prefilter_cap >= 1 && p->prefilter_cap <= 63 && p->texture_threshold >= 0 &&
           p->uniqueness >= 0 && p->uniqueness <= 100 && p->lr_max_diff >= -1 && p->lr_max_diff <= p->num_disp;
}

bool disparity_geometry_ok(int rows, int cols) { return rows > 0 && cols > 0 && cols <= DISP_MAX_COLS; }

extern "C" void viso_disparity_params_default(viso_disparity_params* p) {
    if (!p) return;
    p->num_disp = 128; p->block = 11; p->prefilter_cap = 31; p->texture_threshold = 10; p->uniqueness = 15; p->lr_max_diff = 1;
}

int launch_disparity(hipStream_t s, const StereoImages& im, const viso_disparity_params* p, int16_t* out, size_t ofs) {
    if (im.n <= 0) return VISO_OK;
    DispArgs a;
    a.img = im.img; a.fs = im.fs; a.ss = im.ss; a.out = out; a.ofs = ofs; a.rows = im.rows; a.cols = im.cols; a.p = *p;
    const int K = (p->block + 3) / 4;
    const size_t lds = sizeof(uint32_t) * (size_t)(2 * K + 2) * im.cols;   // <= 14 * 2048 * 4 = 112 KiB
    if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void*)stereo_disparity_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(stereo_disparity_kernel, dim3((unsigned)im.rows, (unsigned)im.n), dim3(DISP_THREADS), lds, s, a);
    HIP_TRY(hipGetLastError());
    return VISO_OK;
}

// The same kernel for one pair of host images on the default context.
extern "C" int viso_stereo_disparity(const uint8_t* left, const uint8_t* right, int rows, int cols, const viso_disparity_params* params,
                                     int16_t* out) {
    if (!left || !right || !out || rows <= 0 || cols <= 0 || !disparity_params_ok(params)) {
        viso_set_error("viso_stereo_disparity: bad argument (non-null images and output, sizes > 0, parameters of include/viso_hip.h)");
        return VISO_ERR_ARG;
    }
    if (!disparity_geometry_ok(rows, cols)) {
        viso_set_error("viso_stereo_disparity: %d columns exceed the %d this build handles", cols, DISP_MAX_COLS);
        return VISO_ERR_UNSUPPORTED;
    }
    const size_t per = (size_t)rows * cols;
    DirectCall dc;
    VISO_TRY(dc.begin());
    uint8_t* dimg; int16_t* dout;
    VISO_TRY(dc.scratch(SLOT_GEN0, 2 * per, &dimg));
    VISO_TRY(dc.scratch(SLOT_GEN1, per, &dout));
    VISO_TRY(dc.up(dimg, left, per));
    VISO_TRY(dc.up(dimg + per, right, per));
    VISO_TRY(launch_disparity(dc.s, image_block(dimg, rows, cols, 0, 1), params, dout, per));
    VISO_TRY(dc.down(out, dout, per));
    return dc.wait();
}
