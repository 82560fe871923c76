// speckle.hip — opt-in speckle filter of the dense disparity maps and their reprojection to 3-D points (NOT in the reference:
// viso_filter_speckles, viso_batch_set_speckle, viso_disparity_to_points, include/viso_hip.h).
//
// The filter removes every 4-connected component of at most max_size pixels, two valid neighbours being linked when their values
// differ by at most max_diff.  Components are found by union-find over labels that are linear pixel indices of the frame; a label
// only ever decreases, so every loop below is bounded by a strictly decreasing index and no workgroup waits for another one.
// Everything is an exact integer: the device output is bit-identical to tests/speckle_ref.py.
//
// Per group of frames (as many as the workspace holds; label [frame][rows * cols] u32, size [frame][rows * cols] u32):
//   speckle_tile_kernel    one workgroup per 64 x 16 tile and frame, the tile in LDS.  A wave per row: the horizontal runs of the row
//                          from one ballot (label = the run's first pixel), then the links to the row above by atomicMin on the
//                          roots in LDS, then every run adds its length to its root's counter in LDS.  Out: label = the tile root
//                          as a frame index, size = the tile component's pixel count at its root and 0 elsewhere.
//   speckle_border_kernel  one thread per pixel of a tile's first column or first row (not the image's): where it is linked to
//                          the pixel across the border, the two roots are joined in device memory by atomicMin on the larger.
//   speckle_count_kernel   one thread per pixel: label = its root (flatten, halving the paths it walks); a tile root that is not the component's root adds
//                          its count to the root's with one integer atomic (one per tile and component, whatever the shape).
//   speckle_apply_kernel   one thread per pixel: invalid where size[label] <= max_size.
//   points_kernel          the reprojection: one thread per pixel, fp64, each coordinate rounded once to f32.
#include "common.h"

#define SPK_TW 64                 // tile width: one wave per tile row
#define SPK_TH 16                 // tile height
#define SPK_THREADS 256
#define SPK_ROWS_PER_WAVE (SPK_TH / (SPK_THREADS / 64))
#define SPK_MAX_DIFF 4096
#define SPK_DEFAULT_CAP ((size_t)2 << 30)
#define SPK_MAX_PIXELS 0x7fffffffll

__device__ __forceinline__ bool spk_linked(int a, int b, int diff) {
    return a != VISO_DISP_INVALID && b != VISO_DISP_INVALID && abs(a - b) <= diff;
}

// ---- union-find on labels in LDS --------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t spk_lds_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ uint32_t spk_lds_find(const uint32_t* lab, uint32_t x) {
    for (uint32_t p = spk_lds_load(lab + x); p < x; p = spk_lds_load(lab + x)) x = p;   // x strictly decreases
    return x;
}

__device__ __forceinline__ void spk_lds_union(uint32_t* lab, uint32_t a, uint32_t b) {
    for (;;) {   // a + b strictly decreases
        a = spk_lds_find(lab, a);
        b = spk_lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(lab + a, b);   // a > b
        if (old == a) return;
        a = old;                                      // a had been linked meanwhile (old < a): join that one with b
    }
}

// ---- union-find on labels in device memory (speckle_border_kernel: other workgroups link at the same time) -------------------
__device__ __forceinline__ uint32_t spk_g_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t spk_g_find(uint32_t* lab, uint32_t x) {
    uint32_t p = spk_g_load(lab + x);
    while (p < x) {                                   // x strictly decreases
        const uint32_t gp = spk_g_load(lab + p);
        if (gp < p) atomicMin(lab + x, gp);           // path halving: gp is an ancestor of x, and atomicMin loses no link
        x = p; p = gp;
    }
    return x;
}

__device__ __forceinline__ void spk_g_union(uint32_t* lab, uint32_t a, uint32_t b) {
    for (;;) {
        a = spk_g_find(lab, a);
        b = spk_g_find(lab, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;
    }
}

struct SpkArgs {
    int16_t* map; size_t mfs;      // frame f's map at map + f * mfs
    uint32_t* lab; uint32_t* siz;  // frame f's words at + f * wfs
    size_t wfs;
    int rows, cols, max_size, max_diff;
};

// ---- the tiles -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SPK_THREADS) void speckle_tile_kernel(SpkArgs a) {
    __shared__ int16_t val[SPK_TH * SPK_TW];
    __shared__ uint32_t lab[SPK_TH * SPK_TW];
    __shared__ uint32_t cnt[SPK_TH * SPK_TW];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.z;
    const int x0 = blockIdx.y * SPK_TW, y0 = blockIdx.x * SPK_TH, rows = a.rows, cols = a.cols, diff = a.max_diff;
    const int16_t* map = a.map + (size_t)f * a.mfs;
    const int x = x0 + lane;
    unsigned long long starts[SPK_ROWS_PER_WAVE];
#pragma unroll
    for (int k = 0; k < SPK_ROWS_PER_WAVE; ++k) {
        const int ry = wave + k * (SPK_THREADS / 64), y = y0 + ry;
        const int v = (x < cols && y < rows) ? (int)map[(size_t)y * cols + x] : VISO_DISP_INVALID;
        const int vl = __shfl_up(v, 1);
        const bool start = lane == 0 || !spk_linked(v, vl, diff);   // the first pixel of a horizontal run (an invalid pixel: a run of its own)
        const unsigned long long m = __ballot(start);
        starts[k] = m;
        const int first = 63 - __clzll((long long)(m & (~0ull >> (63 - lane))));
        val[ry * SPK_TW + lane] = (int16_t)v;
        lab[ry * SPK_TW + lane] = (uint32_t)(ry * SPK_TW + first);
        cnt[ry * SPK_TW + lane] = 0u;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SPK_ROWS_PER_WAVE; ++k) {
        const int ry = wave + k * (SPK_THREADS / 64);
        if (ry > 0 && spk_linked(val[ry * SPK_TW + lane], val[(ry - 1) * SPK_TW + lane], diff))
            spk_lds_union(lab, (uint32_t)(ry * SPK_TW + lane), (uint32_t)((ry - 1) * SPK_TW + lane));
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SPK_ROWS_PER_WAVE; ++k) {
        const int ry = wave + k * (SPK_THREADS / 64);
        const unsigned long long m = starts[k];
        if (((m >> lane) & 1ull) && val[ry * SPK_TW + lane] != VISO_DISP_INVALID) {
            const unsigned long long above = lane < 63 ? m >> (lane + 1) : 0ull;
            const uint32_t len = above ? (uint32_t)__ffsll((long long)above) : (uint32_t)(64 - lane);
            atomicAdd(cnt + spk_lds_find(lab, (uint32_t)(ry * SPK_TW + lane)), len);
        }
    }
    __syncthreads();
    uint32_t* L = a.lab + (size_t)f * a.wfs;
    uint32_t* Z = a.siz + (size_t)f * a.wfs;
#pragma unroll
    for (int k = 0; k < SPK_ROWS_PER_WAVE; ++k) {
        const int ry = wave + k * (SPK_THREADS / 64), y = y0 + ry;
        if (x < cols && y < rows) {
            const uint32_t i = (uint32_t)(ry * SPK_TW + lane);
            const uint32_t r = spk_lds_find(lab, i);
            const uint32_t p = (uint32_t)y * (uint32_t)cols + (uint32_t)x;
            L[p] = (uint32_t)(y0 + (int)(r / SPK_TW)) * (uint32_t)cols + (uint32_t)(x0 + (int)(r % SPK_TW));
            Z[p] = r == i ? cnt[i] : 0u;   // 0 at invalid pixels: no run counted them
        }
    }
}

// ---- the tile borders ------------------------------------------------------------------------------------------------------------
// Items of a frame: first the pixels of the tiles' first columns (x = 64 k, k >= 1; consecutive threads along y), then the pixels of
// the tiles' first rows (y = 16 k, k >= 1; consecutive threads along x).
__global__ __launch_bounds__(256) void speckle_border_kernel(SpkArgs a) {
    const int rows = a.rows, cols = a.cols, f = blockIdx.y;
    const long long nvb = (long long)((cols - 1) / SPK_TW) * rows, nhb = (long long)((rows - 1) / SPK_TH) * cols;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvb + nhb) return;
    int x, y, step;
    if (i < nvb) { x = (int)(i / rows + 1) * SPK_TW; y = (int)(i % rows); step = 1; }
    else { const long long j = i - nvb; y = (int)(j / cols + 1) * SPK_TH; x = (int)(j % cols); step = cols; }
    const int16_t* map = a.map + (size_t)f * a.mfs;
    const uint32_t p = (uint32_t)y * (uint32_t)cols + (uint32_t)x, q = p - (uint32_t)step;
    if (spk_linked(map[p], map[q], a.max_diff)) spk_g_union(a.lab + (size_t)f * a.wfs, p, q);
}

// ---- flatten and count -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void speckle_count_kernel(SpkArgs a) {
    const size_t px = (size_t)a.rows * a.cols, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= px) return;
    uint32_t* L = a.lab + (size_t)blockIdx.y * a.wfs;
    uint32_t* Z = a.siz + (size_t)blockIdx.y * a.wfs;
    const uint32_t p = (uint32_t)i;
    // the walk halves the path it follows (atomicMin with an ancestor), so the chains of tile roots a long thin component leaves
    // behind are shortened by the first threads that meet them; the plain store below writes the root itself, the smallest label
    // of the component, so whichever of the two lands last the word is an ancestor or the root: other threads' walks stay correct
    const uint32_t r = spk_g_find(L, p);
    if (r != p) {
        L[p] = r;
        const uint32_t n = Z[p];            // nobody adds to a pixel that is not a root
        if (n) atomicAdd(Z + r, n);
    }
}

__global__ __launch_bounds__(256) void speckle_apply_kernel(SpkArgs a) {
    const size_t px = (size_t)a.rows * a.cols, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= px) return;
    int16_t* map = a.map + (size_t)blockIdx.y * a.mfs;
    if (map[i] == VISO_DISP_INVALID) return;
    const uint32_t* L = a.lab + (size_t)blockIdx.y * a.wfs;
    const uint32_t* Z = a.siz + (size_t)blockIdx.y * a.wfs;
    if (Z[L[i]] <= (uint32_t)a.max_size) map[i] = (int16_t)VISO_DISP_INVALID;
}

// ---- host: the filter ------------------------------------------------------------------------------------------------------------
bool speckle_geometry_ok(int rows, int cols) { return disparity_geometry_ok(rows, cols) && (long long)rows * cols <= SPK_MAX_PIXELS; }

bool speckle_params_ok(const viso_speckle_params* p) {
    return p && p->max_size >= 0 && p->max_diff >= 0 && p->max_diff <= SPK_MAX_DIFF;
}

extern "C" void viso_speckle_params_default(viso_speckle_params* p) {
    if (!p) return;
    p->max_size = 100; p->max_diff = 16;
}

static WorkspaceCap g_speckle_cap{{SPK_DEFAULT_CAP}, SPK_DEFAULT_CAP, "speckle", "viso_speckle_set_workspace_cap"};

extern "C" void viso_speckle_set_workspace_cap(size_t bytes) { g_speckle_cap.set(bytes); }

size_t speckle_frame_bytes(int rows, int cols) { return 2 * al256((size_t)rows * cols * sizeof(uint32_t)); }

int speckle_group_frames(const char* where, int rows, int cols, int n_frames, int* group) {
    return g_speckle_cap.frames(where, rows, cols, speckle_frame_bytes(rows, cols), n_frames, 16384, group);   // the frames run along the grids' y and z
}

int launch_speckle(hipStream_t s, int16_t* map, size_t mfs, int rows, int cols, int n_frames, const viso_speckle_params* p, void* ws,
                   int group) {
    if (n_frames <= 0 || p->max_size == 0) return VISO_OK;   // max_size 0 removes nothing
    const size_t px = (size_t)rows * cols;
    const size_t half = al256(px * sizeof(uint32_t)) / sizeof(uint32_t);
    SpkArgs a;
    a.rows = rows; a.cols = cols; a.max_diff = p->max_diff;
    a.max_size = (long long)p->max_size > (long long)px ? (int)px : p->max_size;
    a.mfs = mfs; a.wfs = 2 * half;
    a.lab = reinterpret_cast<uint32_t*>(ws); a.siz = a.lab + half;
    const unsigned tx = (unsigned)((cols + SPK_TW - 1) / SPK_TW), ty = (unsigned)((rows + SPK_TH - 1) / SPK_TH);
    const long long borders = (long long)((cols - 1) / SPK_TW) * rows + (long long)((rows - 1) / SPK_TH) * cols;
    const unsigned lin = (unsigned)((px + 255) / 256);
    for (int f0 = 0; f0 < n_frames; f0 += group) {
        const int nf = n_frames - f0 < group ? n_frames - f0 : group;
        a.map = map + (size_t)f0 * mfs;
        hipLaunchKernelGGL(speckle_tile_kernel, dim3(ty, tx, (unsigned)nf), dim3(SPK_THREADS), 0, s, a);   // tile rows along x: any height
        if (borders > 0)
            hipLaunchKernelGGL(speckle_border_kernel, dim3((unsigned)((borders + 255) / 256), (unsigned)nf), dim3(256), 0, s, a);
        hipLaunchKernelGGL(speckle_count_kernel, dim3(lin, (unsigned)nf), dim3(256), 0, s, a);
        hipLaunchKernelGGL(speckle_apply_kernel, dim3(lin, (unsigned)nf), dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
    }
    return VISO_OK;
}

// One host map on the default context, in place.
extern "C" int viso_filter_speckles(int16_t* map, int rows, int cols, const viso_speckle_params* params) {
    if (!map || rows <= 0 || cols <= 0 || !speckle_params_ok(params)) {
        viso_set_error("viso_filter_speckles: bad argument (a non-null map, sizes > 0, max_size >= 0, max_diff in 0..%d)", SPK_MAX_DIFF);
        return VISO_ERR_ARG;
    }
    if (!speckle_geometry_ok(rows, cols)) {
        viso_set_error("viso_filter_speckles: a %d x %d map is beyond this build (2048 columns, 2^31 - 1 pixels)", rows, cols);
        return VISO_ERR_UNSUPPORTED;
    }
    if (params->max_size == 0) return VISO_OK;
    VISO_TRY(speckle_group_frames("viso_filter_speckles", rows, cols, 1, nullptr));
    const size_t per = (size_t)rows * cols;
    DirectCall dc;
    VISO_TRY(dc.begin());
    int16_t* dmap; char* ws;
    VISO_TRY(dc.scratch(SLOT_GEN1, per, &dmap));
    VISO_TRY(dc.scratch(SLOT_GEN2, speckle_frame_bytes(rows, cols), &ws));
    VISO_TRY(dc.up(dmap, map, per));
    VISO_TRY(launch_speckle(dc.s, dmap, per, rows, cols, 1, params, ws, 1));
    VISO_TRY(dc.down(map, dmap, per));
    return dc.wait();
}

// ---- reprojection ----------------------------------------------------------------------------------------------------------------
struct PointsArgs {
    const int16_t* disp; float* out;
    int rows, cols, min_disp16, has_pose;
    double f, cu, cv, base;
    double T[12];   // the pose's first three rows
};

__global__ __launch_bounds__(256) void points_kernel(PointsArgs a) {
    const size_t px = (size_t)a.rows * a.cols, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= px) return;
    const int d16 = a.disp[i];
    float o0 = __builtin_nanf(""), o1 = o0, o2 = o0;
    if (d16 != VISO_DISP_INVALID && d16 >= a.min_disp16) {
        const int y = (int)(i / (size_t)a.cols), x = (int)(i - (size_t)y * a.cols);
        const double d = (double)d16 / 16.0;
        const double X = a.base * ((double)x - a.cu) / d;      // the operand order of triangulate_direct_kernel (circle.hip)
        const double Y = a.base * ((double)y - a.cv) / d;
        const double Z = a.f * a.base / d;
        if (a.has_pose) {
            o0 = (float)(((a.T[0] * X + a.T[1] * Y) + a.T[2] * Z) + a.T[3]);
            o1 = (float)(((a.T[4] * X + a.T[5] * Y) + a.T[6] * Z) + a.T[7]);
            o2 = (float)(((a.T[8] * X + a.T[9] * Y) + a.T[10] * Z) + a.T[11]);
        } else {
            o0 = (float)X; o1 = (float)Y; o2 = (float)Z;
        }
    }
    float* o = a.out + 3 * i;
    o[0] = o0; o[1] = o1; o[2] = o2;
}

int launch_points(hipStream_t s, const DispView& v, int min_disp16, float* out) {
    PointsArgs a;
    a.disp = v.disp; a.out = out; a.rows = v.rows; a.cols = v.cols; a.min_disp16 = min_disp16; a.has_pose = v.poses != nullptr;
    a.f = v.cal.f; a.cu = v.cal.cu; a.cv = v.cal.cv; a.base = v.cal.base;
    for (int k = 0; k < 12; ++k) a.T[k] = v.poses ? v.poses[k] : 0.0;
    hipLaunchKernelGGL(points_kernel, dim3((unsigned)((v.px() + 255) / 256)), dim3(256), 0, s, a);
    HIP_TRY(hipGetLastError());
    return VISO_OK;
}

extern "C" int viso_disparity_to_points(const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_or_null,
                                        int min_disp16, float* out) {
    if (!disp || !out || !param || rows <= 0 || cols <= 0 || min_disp16 < 1) {
        viso_set_error("viso_disparity_to_points: bad argument (non-null map, calibration and output, sizes > 0, min_disp16 >= 1)");
        return VISO_ERR_ARG;
    }
    if ((long long)rows * cols > SPK_MAX_PIXELS) {
        viso_set_error("viso_disparity_to_points: a %d x %d map is beyond this build (2^31 - 1 pixels)", rows, cols);
        return VISO_ERR_UNSUPPORTED;
    }
    const size_t per = (size_t)rows * cols;
    DirectCall dc;
    VISO_TRY(dc.begin());
    int16_t* dmap; float* dout;
    VISO_TRY(dc.scratch(SLOT_GEN1, per, &dmap));
    VISO_TRY(dc.scratch(SLOT_GEN2, 3 * per, &dout));
    VISO_TRY(dc.up(dmap, disp, per));
    DispView v = disp_view_host(disp, nullptr, rows, cols, param, pose_or_null);
    v.disp = dmap;   // this call stages the map itself, in its own scratch
    VISO_TRY(launch_points(dc.s, v, min_disp16, dout));
    VISO_TRY(dc.down(out, dout, 3 * per));
    return dc.wait();
}
