// rectify.hip — opt-in undistortion + stereo rectification of raw camera images (NOT in the reference, which reads KITTI's
// already rectified pairs: viso_rectify_map, viso_batch_set_rectify, include/viso_hip.h; DESIGN.md "Rectification").
//
// A camera's map (mapx, mapy [out_rows][out_cols] float: the raw-image position each output pixel samples) is quantised once
// on the host into one RectEntry per output pixel: the byte offset of its top-left tap, its 1/32-pixel fractions and which of
// its four taps lie inside the raw image.  Outside taps are resolved there, before any address exists: the kernel loads taps
// the entry marks inside and substitutes the border value for the others, so no map can make it read out of bounds.  The
// remap itself is integer bilinear interpolation, exact:
//   out = ((32-fx)(32-fy) t00 + fx(32-fy) t10 + (32-fx) fy t01 + fx fy t11 + 512) >> 10.
#include "common.h"

#include <math.h>
#include <string.h>
#include <vector>

#define RECT_THREADS 256
#define RECT_PX 4               // output pixels per thread: one dword store per image
#define RECT_TILE (RECT_THREADS * RECT_PX)
#define RECT_FPB 32             // frames per workgroup: the map is read once per 32 frames (see rectify_remap_kernel)
#define RECT_PIVOT_U 0.1       // threshold of the map builder's partial pivoting (viso_rectify_map)
#define RECT_IN00 (1u << 10)    // RectEntry::meta bits 10..13: tap (0,0), (1,0), (0,1), (1,1) inside the raw image
#define RECT_IN10 (1u << 11)
#define RECT_IN01 (1u << 12)
#define RECT_IN11 (1u << 13)

// ---- host: the map builder and the quantisation ------------------------------------------------------------------------

// The plumb-bob model in the form of OpenCV's initUndistortRectifyMap, in double (this file builds with -ffp-contract=off).
extern "C" int viso_rectify_map(const double K[9], const double D[5], const double R[9], const double P[12], int out_rows,
                                int out_cols, float* mapx, float* mapy) {
    if (!K || !D || !R || !P || !mapx || !mapy || out_rows <= 0 || out_cols <= 0 || K[1] != 0.0) {
        viso_set_error("viso_rectify_map: bad argument (sizes > 0, non-null pointers, K[0][1] == 0)");
        return VISO_ERR_ARG;
    }
    // The formula of the header, arranged so that K = P33, D = 0, R = I gives the pixel grid exactly: H = Kp (P33 R)^-1 with
    // Kp = [K00 0 K02; 0 K11 K12; 0 0 1], so that (u, v) = (H (x, y, 1)) / w = (K00 x' + K02, K11 y' + K12), and
    // mapx = u + K00 (xd - x'), mapy = v + K11 (yd - y').  H comes from Gauss-Jordan on (P33 R)^T H^T = Kp^T with the pivot row
    // normalised before it is subtracted (a triangular (P33 R) equal to Kp then yields the identity with no rounding).
    // Threshold partial pivoting: the diagonal element stays the pivot while it is at least RECT_PIVOT_U of the column's
    // largest candidate, else the largest is swapped in.  That bounds the growth of the elimination to (1 + 1/u)^3 for any
    // P33 R, and keeps the exact identity for every K whose cx, cy are below 10 fx, 10 fy (the diagonal pivots of Kp^T).
    double A[3][6];   // [(P33 R)^T | Kp^T]
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[j][i] = P[4 * i + 0] * R[j] + P[4 * i + 1] * R[3 + j] + P[4 * i + 2] * R[6 + j];
    const double Kp[3][3] = {{K[0], 0.0, K[2]}, {0.0, K[4], K[5]}, {0.0, 0.0, 1.0}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][3 + j] = Kp[j][i];
    double scale = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) scale = fmax(scale, fabs(A[i][j]));
    for (int c = 0; c < 3; ++c) {
        int best = c;
        for (int i = c + 1; i < 3; ++i)
            if (fabs(A[i][c]) > fabs(A[best][c])) best = i;
        if (!(fabs(A[c][c]) >= RECT_PIVOT_U * fabs(A[best][c])))
            for (int j = 0; j < 6; ++j) { const double t = A[c][j]; A[c][j] = A[best][j]; A[best][j] = t; }
        const double piv = A[c][c];
        if (!(fabs(piv) > 1e-12 * scale) || !isfinite(piv)) { viso_set_error("viso_rectify_map: P33 * R is singular"); return VISO_ERR_ARG; }
        for (int j = 0; j < 6; ++j) A[c][j] = j == c ? 1.0 : A[c][j] / piv;
        for (int i = 0; i < 3; ++i) {
            if (i == c) continue;
            const double f = A[i][c];
            for (int j = 0; j < 6; ++j) A[i][j] = j == c ? 0.0 : A[i][j] - f * A[c][j];
        }
    }
    double H[3][3];   // H^T is the right half
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) H[j][i] = A[i][3 + j];
    const double k1 = D[0], k2 = D[1], p1 = D[2], p2 = D[3], k3 = D[4];
    const double fx = K[0], cx = K[2], fy = K[4], cy = K[5];
    for (int y = 0; y < out_rows; ++y)
        for (int x = 0; x < out_cols; ++x) {
            const double w = H[2][0] * x + H[2][1] * y + H[2][2];
            const double u = (H[0][0] * x + H[0][1] * y + H[0][2]) / w, v = (H[1][0] * x + H[1][1] * y + H[1][2]) / w;
            const double xp = (u - cx) / fx, yp = (v - cy) / fy;
            const double r2 = xp * xp + yp * yp;
            const double kr1 = k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2;   // kr - 1
            const double dx = xp * kr1 + 2.0 * p1 * xp * yp + p2 * (r2 + 2.0 * xp * xp);
            const double dy = yp * kr1 + p1 * (r2 + 2.0 * yp * yp) + 2.0 * p2 * xp * yp;
            mapx[(size_t)y * out_cols + x] = (float)(u + fx * dx);
            mapy[(size_t)y * out_cols + x] = (float)(v + fy * dy);
        }
    return VISO_OK;
}

// The quantisation of the header: X = lrintf(mapx * 32) (nearest, ties to even; the product is exact), ix = floor(X / 32),
// fx = X & 31; an entry that is not finite or has |map| >= 32768 is outside (border, no load).  Geometry limits are checked by
// the callers (rect_geometry_ok).
void rect_quantise(const float* mapx, const float* mapy, size_t n, int raw_rows, int raw_cols, RectEntry* out) {
    for (size_t i = 0; i < n; ++i) {
        const float mx = mapx[i], my = mapy[i];
        RectEntry e = {0, 0u};
        if (isfinite(mx) && isfinite(my) && fabsf(mx) < 32768.f && fabsf(my) < 32768.f) {
            const long X = lrintf(mx * 32.f), Y = lrintf(my * 32.f);
            const int fx = (int)(X & 31), fy = (int)(Y & 31);
            const long ix = (X - fx) / 32, iy = (Y - fy) / 32;
            const bool x0 = ix >= 0 && ix < raw_cols, x1 = ix + 1 >= 0 && ix + 1 < raw_cols;
            const bool y0 = iy >= 0 && iy < raw_rows, y1 = iy + 1 >= 0 && iy + 1 < raw_rows;
            const unsigned in = (x0 && y0 ? RECT_IN00 : 0u) | (x1 && y0 ? RECT_IN10 : 0u) | (x0 && y1 ? RECT_IN01 : 0u) |
                                (x1 && y1 ? RECT_IN11 : 0u);
            if (in) {   // every inside tap's offset is then in [0, raw_rows * raw_cols)
                e.off = (int)(iy * raw_cols + ix);
                e.meta = (unsigned)fx | ((unsigned)fy << 5) | in;
            }
        }
        out[i] = e;
    }
}

bool rect_geometry_ok(int raw_rows, int raw_cols, int out_rows, int out_cols) {
    return raw_rows > 0 && raw_cols > 0 && out_rows > 0 && out_cols > 0 &&
           (long long)raw_rows * raw_cols + raw_cols + 2 < (1ll << 31) && (long long)out_rows * out_cols < (1ll << 31);
}

// ---- device: the remap ----------------------------------------------------------------------------------------------------

// Image (f, side) of the source is raw + f * raw_fs + side * raw_ss, of the destination out + f * out_fs + side * out_ss; the
// map of side s is map + s * per.  Grid: (tiles of RECT_TILE output pixels, sides, chunks of RECT_FPB frames).
struct RectArgs {
    const uint8_t* raw; size_t raw_fs, raw_ss;
    uint8_t* out; size_t out_fs, out_ss;
    const RectEntry* map; int per;
    int n_frames; int border;
};

// A workgroup owns RECT_TILE consecutive output pixels of one side (a strip of the row-major image: the raw bytes its taps
// read are a band of a few raw rows, L1/L2-resident).  Each thread loads the RectEntry of its RECT_PX pixels into registers
// once, then loops over its chunk of the launch's frames: 4 byte gathers per pixel, integer arithmetic, one dword store per frame
// (DWORD: every image base and the tile are 4-byte aligned, i.e. out_rows * out_cols % 4 == 0; else byte stores).  Chunks of
// RECT_FPB frames, not the whole upload: one workgroup per tile and side left the GPU at 3.5 waves per SIMD, each wave walking
// 513 frames one dependent gather round after the other (1.64 ms for 1 026 images); the chunks fill it, and the
// maps are still read once per 32 frames instead of once per image.
template <bool DWORD>
__global__ __launch_bounds__(RECT_THREADS) void rectify_remap_kernel(RectArgs a, int raw_cols) {
    typedef const __attribute__((address_space(1))) uint8_t* gbyte_t;
    const int side = blockIdx.y;
    const long long p0 = ((long long)blockIdx.x * RECT_THREADS + threadIdx.x) * RECT_PX;
    const RectEntry* mp = a.map + (size_t)side * a.per;
    int off[RECT_PX]; unsigned meta[RECT_PX];
#pragma unroll
    for (int k = 0; k < RECT_PX; ++k) {
        RectEntry e = {0, 0u};   // past the image: border, never stored
        if (p0 + k < a.per) e = mp[p0 + k];
        off[k] = e.off; meta[k] = e.meta;
    }
    const uint32_t border = (uint32_t)a.border;
    const int W = raw_cols;
    const int f_end = min(a.n_frames, (int)(blockIdx.z + 1) * RECT_FPB);
    for (int f = blockIdx.z * RECT_FPB; f < f_end; ++f) {
        gbyte_t src = (gbyte_t)(a.raw + (size_t)f * a.raw_fs + (size_t)side * a.raw_ss);
        uint32_t v[RECT_PX][4];
#pragma unroll
        for (int k = 0; k < RECT_PX; ++k) {   // all 16 loads first: the gathers of a frame are in flight together
            const int o = off[k];
            const unsigned m = meta[k];
            v[k][0] = src[(m & RECT_IN00) ? o : 0];
            v[k][1] = src[(m & RECT_IN10) ? o + 1 : 0];
            v[k][2] = src[(m & RECT_IN01) ? o + W : 0];
            v[k][3] = src[(m & RECT_IN11) ? o + W + 1 : 0];
        }
        uint32_t word = 0;
#pragma unroll
        for (int k = 0; k < RECT_PX; ++k) {
            const unsigned m = meta[k];
            const uint32_t fx = m & 31u, fy = (m >> 5) & 31u;
            const uint32_t t00 = (m & RECT_IN00) ? v[k][0] : border, t10 = (m & RECT_IN10) ? v[k][1] : border;
            const uint32_t t01 = (m & RECT_IN01) ? v[k][2] : border, t11 = (m & RECT_IN11) ? v[k][3] : border;
            const uint32_t s = (32u - fx) * (32u - fy) * t00 + fx * (32u - fy) * t10 + (32u - fx) * fy * t01 + fx * fy * t11 + 512u;
            word |= (s >> 10) << (8 * k);
        }
        uint8_t* dst = a.out + (size_t)f * a.out_fs + (size_t)side * a.out_ss;
        if (DWORD && p0 + RECT_PX <= a.per) {
            *reinterpret_cast<uint32_t*>(dst + p0) = word;
        } else {
#pragma unroll
            for (int k = 0; k < RECT_PX; ++k)
                if (p0 + k < a.per) dst[p0 + k] = (uint8_t)(word >> (8 * k));
        }
    }
}

int launch_rectify(hipStream_t s, const StereoImages& raw, const StereoImages& out, const RectEntry* map, int border) {
    if (out.n <= 0) return VISO_OK;
    RectArgs a;
    a.raw = raw.img; a.raw_fs = raw.fs; a.raw_ss = raw.ss;
    a.out = out.img; a.out_fs = out.fs; a.out_ss = out.ss;
    a.map = map; a.per = out.rows * out.cols;
    a.n_frames = out.n; a.border = border;
    const dim3 grid((unsigned)((a.per + RECT_TILE - 1) / RECT_TILE), out.ss ? 2u : 1u, (unsigned)((out.n + RECT_FPB - 1) / RECT_FPB));
    const bool dw = (a.per % 4 == 0) && (out.fs % 4 == 0) && (out.ss % 4 == 0) && ((uintptr_t)out.img % 4 == 0);
    if (dw) hipLaunchKernelGGL(rectify_remap_kernel<true>, grid, dim3(RECT_THREADS), 0, s, a, raw.cols);
    else hipLaunchKernelGGL(rectify_remap_kernel<false>, grid, dim3(RECT_THREADS), 0, s, a, raw.cols);
    HIP_TRY(hipGetLastError());
    return VISO_OK;
}

// The same kernel for host pointers on the default context: n raw images of one camera -> n rectified images.
extern "C" int viso_rectify_images(const uint8_t* raw, int n, int raw_rows, int raw_cols, const float* mapx, const float* mapy,
                                   int out_rows, int out_cols, int border, uint8_t* out) {
    if (n < 0 || !rect_geometry_ok(raw_rows, raw_cols, out_rows, out_cols) || border < 0 || border > 255 || !mapx || !mapy ||
        (n && (!raw || !out))) {
        viso_set_error("viso_rectify_images: bad argument (sizes > 0, border 0..255, non-null maps)");
        return VISO_ERR_ARG;
    }
    if (n == 0) return VISO_OK;
    const size_t rper = (size_t)raw_rows * raw_cols, oper = (size_t)out_rows * out_cols;
    std::vector<RectEntry> q(oper);
    rect_quantise(mapx, mapy, oper, raw_rows, raw_cols, q.data());
    DirectCall dc;
    VISO_TRY(dc.begin());
    uint8_t *draw, *dout; RectEntry* dmap;
    VISO_TRY(dc.scratch(SLOT_RECT_RAW, rper * (size_t)n, &draw));
    VISO_TRY(dc.scratch(SLOT_RECT_OUT, oper * (size_t)n, &dout));
    VISO_TRY(dc.scratch(SLOT_RECT_MAP, oper, &dmap));
    VISO_TRY(dc.up(draw, raw, rper * (size_t)n));
    VISO_TRY(dc.up(dmap, q.data(), oper));
    VISO_TRY(launch_rectify(dc.s, image_block(draw, raw_rows, raw_cols, 0, n, 1), image_block(dout, out_rows, out_cols, 0, n, 1), dmap, border));
    VISO_TRY(dc.down(out, dout, oper * (size_t)n));
    return dc.wait();
}
