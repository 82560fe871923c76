// subpixel.hip — opt-in sub-pixel refinement of the stereo observations (NOT in the reference: viso_batch_set_subpixel,
// include/viso_hip.h; DESIGN.md "Sub-pixel stereo refinement").  For a stereo row (i1, i2, dist) with p = cvRound(kp1[i1]),
// q = cvRound(kp2[i2]): the SADs of the left descriptor window W_L(p) against the right windows at q + (d, 0) and
// q + (0, d), d in {-1, 0, 1} -- MyFeatureExtractor's 11x11 Sobel-x window (src/viso.cpp:1004-1024) at a shifted keypoint --
// and a parabola through each triple of costs: uR' = q.x + off(Sx), vR' = q.y + off(Sy) (mode 2) or q.y (mode 1).
//
// In a batch the left window is the left keypoint's packed u16 row (the image-in run's extract_pack_kernel wrote it); the right
// windows are recomputed from the resident right image: one 15 x 15 byte region per row gives all five.  Integer SADs, double
// only in the final division; details at subpixel_refine_kernel.
#include "common.h"
#include "wave.h"

#define SUBPIX_THREADS 256
#define SUBPIX_WPB (SUBPIX_THREADS / 64)
#define SUBPIX_GPW 4            // stereo rows per wave at a time: one per 16-lane DPP row of the wave
#define SUBPIX_R 15             // right region: 15 x 15 bytes = the five windows' Sobel centres (13 x 13) + the stencil's ring
#define SUBPIX_RS 20            // bytes per staged right-region row: five dwords cover any alignment of 15 bytes
#define SUBPIX_S 13             // right Sobel grid: centres (q.y - 6 .. q.y + 6) x (q.x - 6 .. q.x + 6)
#define SUBPIX_L 13             // left region (host-pointer entry only): the 11 x 11 window + the ring
#define SUBPIX_BLOCKS_PER_FRAME 16

__device__ __forceinline__ int subpix_reflect101(int p, int len) {   // only called for p in [0, len]
    if (len == 1) return 0;
    return p < len ? p : 2 * len - 2 - p;
}

// Point2i p = kp.pt (src/viso.cpp:1013): rint (half to even) of the float; the integer used for addressing is clamped so that
// far-away coordinates cannot overflow (their windows are all zero either way), the float is what the output is built on.
__device__ __forceinline__ int subpix_addr(float r) { return (int)fminf(fmaxf(r, -1073741824.f), 1073741824.f); }

// off(S-, S0, S+) of the header: the vertex of the parabola through the three costs when S0 is a minimum and the costs curve
// upward, else 0 (|off| <= 1/2)
__device__ __forceinline__ double subpix_off(int sm, int s0, int sp) {
    const int den = sm + sp - 2 * s0;
    if (s0 <= sm && s0 <= sp && den > 0) return (double)(sm - sp) / (2.0 * (double)den);
    return 0.0;
}

// LDS written by some lanes of the wave, read by others: the order made explicit (wavefront-scope release / acquire around
// the wave barrier)
__device__ __forceinline__ void subpix_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Sum over the 16 lanes of a DPP row: lane 15 of the row holds it (row_shr 1, 2, 4, 8: an inclusive scan inside the row)
__device__ __forceinline__ uint32_t subpix_row_sum(uint32_t v) {
    v += viso_dpp<0x111, 0xf>(v, 0u);
    v += viso_dpp<0x112, 0xf>(v, 0u);
    v += viso_dpp<0x114, 0xf>(v, 0u);
    v += viso_dpp<0x118, 0xf>(v, 0u);
    return v;
}

// Frame t (blockIdx.y): left image images + t * img_stride, right image r_off bytes behind it; keypoints kp + t * kp_stride
// (left) and cap entries behind them (right); stereo list lists + t * list_stride with m_cnt[t] rows; output uv + t * cap.
// Batches (lrows != null): W_L is the left keypoint's packed u16 row (extract_pack_kernel wrote it this run), lrows +
// t * lrows_stride at bucket-order position lrank[t * lrank_stride + i1].  Host-pointer calls: W_L from the left image.
struct SubpixArgs {
    const uint8_t* images; size_t img_stride, r_off; int rows, cols;
    const float2* kp; size_t kp_stride; int cap;
    const int* lists; size_t list_stride; const int* m_cnt;
    const uint16_t* lrows; size_t lrows_stride; const int* lrank; size_t lrank_stride;
    float2* uv;
    int mode;
};

// One 16-lane DPP row per stereo row, four per wave.  The right region of a row is fetched as five dwords per image row
// (interior regions; byte gathers with BORDER_REFLECT_101 near the border), each distinct Sobel centre of the five windows
// is computed once into LDS (13 x 13), and lane l of the row owns window elements 8l .. 8l + 7: the left ones in registers
// (one 16-byte load of the packed row), the five right ones of each from the grid.  The five SADs are summed across the 16
// lanes with DPP; lane 15 does the two double divisions.  No atomics: a row's output depends on that row alone.
template <bool LROWS>
__global__ __launch_bounds__(SUBPIX_THREADS) void subpixel_refine_kernel(SubpixArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char s_r[SUBPIX_WPB * SUBPIX_GPW][SUBPIX_R * SUBPIX_RS];
    __shared__ short s_sob[SUBPIX_WPB * SUBPIX_GPW][SUBPIX_S * SUBPIX_S + 1];
    __shared__ unsigned char s_l[LROWS ? 1 : SUBPIX_WPB * SUBPIX_GPW][SUBPIX_L * SUBPIX_L + 3];
    typedef const __attribute__((address_space(1))) uint8_t* gbyte_t;
    typedef const __attribute__((address_space(1))) uint32_t* gword_t;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int g = lane >> 4, l = lane & 15;
    const int slot = wv * SUBPIX_GPW + g;
    const int t = blockIdx.y;
    const int M = min(a.m_cnt[t], a.cap);
    const int rows = a.rows, cols = a.cols;
    const uint8_t* imL = a.images + (size_t)t * a.img_stride;
    const uint8_t* imR = imL + a.r_off;
    const float2* kp1 = a.kp + (size_t)t * a.kp_stride;
    const float2* kp2 = kp1 + a.cap;
    const int* list = a.lists + (size_t)t * a.list_stride;
    const bool vert = a.mode == 2;
    unsigned char* sr = s_r[slot];
    short* sob = s_sob[slot];
    for (int r0 = (blockIdx.x * SUBPIX_WPB + wv) * SUBPIX_GPW; r0 < M; r0 += gridDim.x * SUBPIX_WPB * SUBPIX_GPW) {
        const int r = r0 + g;
        const bool act = r < M;
        int i1 = 0, i2 = 0;
        float2 k1 = make_float2(0.f, 0.f), k2 = make_float2(0.f, 0.f);
        if (act) { i1 = list[3 * r]; i2 = list[3 * r + 1]; k1 = kp1[i1]; k2 = kp2[i2]; }
        const float qxf = rintf(k2.x), qyf = rintf(k2.y);
        const int px = subpix_addr(rintf(k1.x)), py = subpix_addr(rintf(k1.y));
        const int qx = subpix_addr(qxf), qy = subpix_addr(qyf);
        // left window elements 8l .. 8l + 7 of this lane
        int L[8];
        if (LROWS) {
            uint4 w = make_uint4(VISO_BIAS | (VISO_BIAS << 16), VISO_BIAS | (VISO_BIAS << 16), VISO_BIAS | (VISO_BIAS << 16), VISO_BIAS | (VISO_BIAS << 16));
            if (act) {
                const uint16_t* row = a.lrows + (size_t)t * a.lrows_stride + (size_t)a.lrank[(size_t)t * a.lrank_stride + i1] * VISO_ROW;
                w = reinterpret_cast<const uint4*>(row)[l];
            }
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) L[j] = (int)((ww[j >> 1] >> (16 * (j & 1))) & 0xffffu) - VISO_BIAS;
        }
        // the right region (qy - 7 .. qy + 7) x (qx - 7 .. qx + 7).  Interior (every region row but the image's last, whole
        // columns inside): row rr as the five aligned dwords that hold its 15 bytes, the row's bytes start at sh(rr).  Else byte
        // by byte at offset 0: a Sobel centre inside the image (0 < y < rows, 0 < x < cols) reads rows 0..rows and columns
        // 0..cols, of which only `rows` and `cols` themselves need the reflection; every other byte is never read by a centre
        // that counts
        const bool fast = qx >= 7 && qx + 7 < cols && qy >= 7 && qy + 7 < rows - 1;
        const size_t off0 = fast ? (size_t)(qy - 7) * cols + (size_t)(qx - 7) + (size_t)(imR - a.images) : 0;
        if (act && fast) {
            const int s0 = (int)(off0 & 3);
            const gword_t wbase = (gword_t)(a.images + (off0 - s0));
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int e = l + 16 * u;                                  // 75 dwords: (region row, dword)
                if (e < SUBPIX_R * 5) {
                    const int rr = e / 5, j = e - rr * 5;
                    const int sh = (s0 + rr * (cols & 3)) & 3;             // alignment of region row rr
                    const size_t rowoff = (size_t)rr * cols + (size_t)s0 - (size_t)sh;   // aligned start of row rr, from wbase
                    reinterpret_cast<uint32_t*>(sr)[rr * (SUBPIX_RS / 4) + j] = wbase[rowoff / 4 + j];
                }
            }
        } else if (act) {
            const gbyte_t im = (gbyte_t)imR;
#pragma unroll 5
            for (int u = 0; u < 15; ++u) {
                const int e = l + 16 * u;
                if (e < SUBPIX_R * SUBPIX_R) {
                    const int rr = e / SUBPIX_R, cc = e - rr * SUBPIX_R;
                    const int y = qy - 7 + rr, x = qx - 7 + cc;
                    unsigned char v = 0;
                    if (y >= 0 && y <= rows && x >= 0 && x <= cols) v = im[(size_t)subpix_reflect101(y, rows) * cols + subpix_reflect101(x, cols)];
                    sr[rr * SUBPIX_RS + cc] = v;
                }
            }
        }
        if (!LROWS && act) {   // host-pointer entry: the left region byte by byte
            const gbyte_t im = (gbyte_t)imL;
            unsigned char* sl = s_l[LROWS ? 0 : slot];
            for (int e = l; e < SUBPIX_L * SUBPIX_L; e += 16) {
                const int wy = e / SUBPIX_L, wx = e - wy * SUBPIX_L;
                const int y = py - 6 + wy, x = px - 6 + wx;
                unsigned char v = 0;
                if (y >= 0 && y <= rows && x >= 0 && x <= cols) v = im[(size_t)subpix_reflect101(y, rows) * cols + subpix_reflect101(x, cols)];
                sl[e] = v;
            }
        }
        subpix_wave_sync();
        // every distinct Sobel centre of the five right windows, zeroed where y<=0 | y>=rows | x<=0 | x>=cols (src/viso.cpp:1018)
        if (act) {
            const int s0 = fast ? (int)(off0 & 3) : 0;
            for (int e = l; e < SUBPIX_S * SUBPIX_S; e += 16) {
                const int cy = e / SUBPIX_S, cx = e - cy * SUBPIX_S;
                const int y = qy - 6 + cy, x = qx - 6 + cx;
                int v = 0;
                if (y > 0 && y < rows && x > 0 && x < cols) {
                    const int rr = cy + 1, cc = cx + 1;   // region row / column of the centre
                    const unsigned char* r0 = sr + (rr - 1) * SUBPIX_RS + (fast ? (s0 + (rr - 1) * (cols & 3)) & 3 : 0) + cc;
                    const unsigned char* r1 = sr + rr * SUBPIX_RS + (fast ? (s0 + rr * (cols & 3)) & 3 : 0) + cc;
                    const unsigned char* r2 = sr + (rr + 1) * SUBPIX_RS + (fast ? (s0 + (rr + 1) * (cols & 3)) & 3 : 0) + cc;
                    v = ((int)r0[1] - (int)r0[-1]) + 2 * ((int)r1[1] - (int)r1[-1]) + ((int)r2[1] - (int)r2[-1]);
                }
                sob[e] = (short)v;
            }
            if (!LROWS) {
                const unsigned char* sl = s_l[LROWS ? 0 : slot];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = 8 * l + j;
                    L[j] = 0;
                    if (c < 121) {
                        const int ey = c / 11, ex = c - ey * 11;
                        const int y = py + ey - 5, x = px + ex - 5;
                        if (y > 0 && y < rows && x > 0 && x < cols) {
                            const unsigned char* r0 = sl + ey * SUBPIX_L + ex;   // centre = (ey + 1, ex + 1)
                            const unsigned char* r1 = r0 + SUBPIX_L;
                            const unsigned char* r2 = r1 + SUBPIX_L;
                            L[j] = ((int)r0[2] - (int)r0[0]) + 2 * ((int)r1[2] - (int)r1[0]) + ((int)r2[2] - (int)r2[0]);
                        }
                    }
                }
            }
        }
        subpix_wave_sync();
        // S[0..2] = Sx(-1, 0, +1), S[3], S[4] = Sy(-1), Sy(+1); element (ey, ex) of W_R(q + (dx, dy)) = grid (ey + 1 + dy, ex + 1 + dx)
        uint32_t S[5] = {0, 0, 0, 0, 0};
        if (act) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = 8 * l + j;
                if (c < 121) {
                    const int ey = c / 11, ex = c - ey * 11;
                    const short* p0 = sob + (ey + 1) * SUBPIX_S + ex + 1;
                    S[0] += (uint32_t)abs(L[j] - (int)p0[-1]);
                    S[1] += (uint32_t)abs(L[j] - (int)p0[0]);
                    S[2] += (uint32_t)abs(L[j] - (int)p0[1]);
                    if (vert) {
                        S[3] += (uint32_t)abs(L[j] - (int)p0[-SUBPIX_S]);
                        S[4] += (uint32_t)abs(L[j] - (int)p0[SUBPIX_S]);
                    }
                }
            }
        }
        int tot[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) tot[m] = (m >= 3 && !vert) ? 0 : (int)subpix_row_sum(S[m]);   // <= 121 * 2040: exact in 32 bits
        if (act && l == 15) {
            const float u = (float)((double)qxf + subpix_off(tot[0], tot[1], tot[2]));
            // q is an integer in the header: rintf gives -0 for a keypoint in [-0.5, -0], and + 0.f makes it the +0 of mode 2
            const float v = vert ? (float)((double)qyf + subpix_off(tot[3], tot[1], tot[4])) : qyf + 0.f;
            a.uv[(size_t)t * a.cap + r] = make_float2(u, v);
        }
        subpix_wave_sync();   // the next rows' staging rewrites s_r / s_sob
    }
}

int launch_subpixel(hipStream_t s, const StereoImages& im, const SubpixLists& l, int mode, float2* uv, const SubpixLeftRows& left) {
    if (im.n <= 0 || l.cap <= 0) return VISO_OK;
    SubpixArgs a;
    a.images = im.img; a.img_stride = im.fs; a.r_off = im.ss; a.rows = im.rows; a.cols = im.cols;
    a.kp = l.kp; a.kp_stride = l.kp_stride; a.cap = l.cap;
    a.lists = l.lists; a.list_stride = l.list_stride; a.m_cnt = l.m_cnt;
    a.lrows = left.lrows; a.lrows_stride = left.lrows_stride; a.lrank = left.lrank; a.lrank_stride = left.lrank_stride;
    a.uv = uv; a.mode = mode;
    const int per_block = SUBPIX_WPB * SUBPIX_GPW;
    const int gx = min(SUBPIX_BLOCKS_PER_FRAME, (l.cap + per_block - 1) / per_block);
    if (left.lrows) hipLaunchKernelGGL(subpixel_refine_kernel<true>, dim3(gx, im.n), dim3(SUBPIX_THREADS), 0, s, a);
    else hipLaunchKernelGGL(subpixel_refine_kernel<false>, dim3(gx, im.n), dim3(SUBPIX_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    return VISO_OK;
}

// The same device code for host pointers on the default context (single calls, tests): both images and both keypoint sets
// are staged into scratch blocks laid out like one frame of a batch.
extern "C" int viso_refine_stereo_subpixel(const uint8_t* imgL, const uint8_t* imgR, int rows, int cols, const float* kp1, int n1,
                                           const float* kp2, int n2, const int32_t* match, int n, int mode, float* out_uv) {
    if (!imgL || !imgR || rows <= 0 || cols <= 0 || n1 < 0 || n2 < 0 || n < 0 || (mode != 1 && mode != 2) ||
        (n && (!kp1 || !kp2 || !match || !out_uv))) {
        viso_set_error("viso_refine_stereo_subpixel: bad argument (mode must be 1 or 2)");
        return VISO_ERR_ARG;
    }
    for (int i = 0; i < n; ++i)
        if (match[3 * i] < 0 || match[3 * i] >= n1 || match[3 * i + 1] < 0 || match[3 * i + 1] >= n2) {
            viso_set_error("viso_refine_stereo_subpixel: match row %d indexes outside the keypoints", i);
            return VISO_ERR_ARG;
        }
    if (n == 0) return VISO_OK;
    DirectCall dc;
    VISO_TRY(dc.begin());
    const size_t per = (size_t)rows * cols;
    const int cap = n1 > n2 ? n1 : n2;
    const int capn = cap > n ? cap : n;
    uint8_t* dimg; float2* dkp; int* dlist; float2* duv;
    VISO_TRY(dc.scratch(SLOT_SUBPIX_IMG, 2 * per, &dimg));
    VISO_TRY(dc.scratch(SLOT_SUBPIX_KP, 2 * (size_t)capn, &dkp));
    VISO_TRY(dc.scratch(SLOT_SUBPIX_LIST, 3 * (size_t)n + 1, &dlist));
    VISO_TRY(dc.scratch(SLOT_SUBPIX_UV, (size_t)capn, &duv));
    VISO_TRY(dc.up(dimg, imgL, per));
    VISO_TRY(dc.up(dimg + per, imgR, per));
    VISO_TRY(dc.up(dkp, kp1, 2 * (size_t)n1));
    VISO_TRY(dc.up(dkp + capn, kp2, 2 * (size_t)n2));
    VISO_TRY(dc.up(dlist, match, 3 * (size_t)n));
    VISO_TRY(dc.up(dlist + 3 * (size_t)n, &n, 1));
    const SubpixLists lists = {dkp, 2 * (size_t)capn, capn, dlist, 3 * (size_t)n, dlist + 3 * (size_t)n};
    VISO_TRY(launch_subpixel(dc.s, image_block(dimg, rows, cols, 0, 1), lists, mode, duv));
    VISO_TRY(dc.down(out_uv, duv, 2 * (size_t)n));
    return dc.wait();
}
