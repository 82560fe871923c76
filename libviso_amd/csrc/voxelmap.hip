// voxelmap.hip — opt-in voxel map: dense disparity maps and poses fused into a hash table of voxels on the device (NOT in the
// reference: viso_map_*, viso_batch_fuse_disparities, include/viso_hip.h).
//
// The table is open addressing over 2^capacity_log2 slots: keys [slots] u64 (all ones = empty), cnt [slots] u32, sums [slots][3] u64.
// A key is claimed with one 64-bit compare-and-swap; everything added behind it is an integer atomic add, so the table after any
// set of calls depends on neither their order nor on scheduling (only WHICH slot a voxel sits in does, and the getter sorts).
// Every probe loop is bounded by the capacity and advances strictly; no workgroup waits for another one.
//
//   map_fuse_kernel         one thread per pixel of a group of frames, fp64 up to the one division and floor of the definition.  Lanes
//                           that continue the key of the lane to their left form a run: the run heads from one ballot, the runs' offset
//                           sums from two wave scans (DPP) of the packed offsets and one exchange with the run's last lane.  Only the
//                           head lane probes the table and issues the four atomic adds (count, three sums).
//   map_add_entries_kernel  one thread per entry through the same probe.
//   map_compact_kernel      one thread per slot: the occupied slots with count >= min_count to a dense list, one atomic per wave for
//                           the list positions (out == null: only their number).
//   map_clear_kernel        one thread per slot.
// The statistics are 256 sets of counters on cache lines of their own (a workgroup adds to set blockIdx & 255, one atomic per wave
// and counter), summed on the host; the dropped points, which are rare, have one word.
#include "common.h"
#include "voxel_hash.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <unordered_set>
#include <vector>

#define MAP_STAT_SETS 256
#define MAP_STAT_WORDS 16               // 128 bytes a set
#define MAP_ST_POINTS 0
#define MAP_ST_INSERTS 1
#define MAP_ST_OOR 2
#define MAP_ST_OCC 3
#define MAP_W_OUT 0                     // words: the compaction's list length
#define MAP_W_DROPPED 1                 //        points that found no slot
#define MAP_MAX_PIXELS 0x7fffffffll
#define MAP_GROUP 16384                 // frames along a grid's y

struct MapTable {
    unsigned long long* keys; uint32_t* cnt; unsigned long long* sums;
    unsigned long long* stats;   // [MAP_STAT_SETS][MAP_STAT_WORDS]
    unsigned long long* words;   // MAP_W_*
    uint32_t mask;               // slots - 1
};

// count points with offset sums sx, sy, sz into the voxel `key`
__device__ __forceinline__ void map_insert(const MapTable& t, unsigned long long key, uint32_t count, unsigned long long sx,
                                           unsigned long long sy, unsigned long long sz, bool* claimed) {
    uint32_t slot;
    if (voxel_probe(t.keys, t.mask, key, &slot, claimed)) {
        atomicAdd(t.cnt + slot, count);
        atomicAdd(t.sums + 3 * (size_t)slot + 0, sx);
        atomicAdd(t.sums + 3 * (size_t)slot + 1, sy);
        atomicAdd(t.sums + 3 * (size_t)slot + 2, sz);
    } else {
        atomicAdd(t.words + MAP_W_DROPPED, (unsigned long long)count);
    }
}

// One atomic per wave and counter that is not zero; every lane of the wave calls.
__device__ __forceinline__ void map_count_wave(const MapTable& t, unsigned block, int lane, bool points, bool inserts, bool oor, bool occ) {
    const unsigned long long np = __popcll(__ballot(points)), ni = __popcll(__ballot(inserts));
    const unsigned long long no = __popcll(__ballot(oor)), nc = __popcll(__ballot(occ));
    if (lane == 0) {
        unsigned long long* st = t.stats + (size_t)(block & (MAP_STAT_SETS - 1)) * MAP_STAT_WORDS;
        if (np) atomicAdd(st + MAP_ST_POINTS, np);
        if (ni) atomicAdd(st + MAP_ST_INSERTS, ni);
        if (no) atomicAdd(st + MAP_ST_OOR, no);
        if (nc) atomicAdd(st + MAP_ST_OCC, nc);
    }
}

struct FuseArgs {
    const int16_t* disp; size_t mfs;   // frame f's map at disp + f * mfs
    const double* poses;               // [frames][12] on the device, or null: no transform
    int rows, cols, min_disp16, _pad;
    double f, cu, cv, base, s;
    MapTable t;
};

__global__ __launch_bounds__(256) void map_fuse_kernel(FuseArgs a) {
    const size_t px = (size_t)a.rows * a.cols, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, fr = blockIdx.y;
    unsigned long long key = MAP_EMPTY;
    uint32_t oxy = 0, oz = 0;     // ox | oy << 16: a wave's sums stay below 2^16 a field (64 x 1023)
    bool point = false, oor = false;
    if (i < px) {
        const int d16 = a.disp[(size_t)fr * a.mfs + i];
        if (d16 != VISO_DISP_INVALID && d16 >= a.min_disp16) {
            point = true;
            const int y = (int)(i / (size_t)a.cols), x = (int)(i - (size_t)y * a.cols);
            const double d = (double)d16 / 16.0;
            double X = a.base * ((double)x - a.cu) / d;      // the operand order of points_kernel (speckle.hip)
            double Y = a.base * ((double)y - a.cv) / d;
            double Z = a.f * a.base / d;
            if (a.poses) {
                const double* T = a.poses + (size_t)fr * 12;
                const double p0 = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
                const double p1 = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
                const double p2 = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
                X = p0; Y = p1; Z = p2;
            }
            const double gx = floor(X / a.s), gy = floor(Y / a.s), gz = floor(Z / a.s);
            if (fabs(gx) < MAP_RANGE && fabs(gy) < MAP_RANGE && fabs(gz) < MAP_RANGE) {   // false for a NaN
                const int ix = (int)gx, iy = (int)gy, iz = (int)gz;
                key = map_key(ix >> 10, iy >> 10, iz >> 10);
                oxy = (uint32_t)(ix & 1023) | ((uint32_t)(iy & 1023) << 16);
                oz = (uint32_t)(iz & 1023);
            } else {
                oor = true;
            }
        }
    }
    // the runs of equal keys along the wave (lanes without a point: runs of the empty key, which insert nothing)
    const unsigned long long kl = __shfl_up(key, 1);
    const bool head = lane == 0 || key != kl;
    const unsigned long long m = __ballot(head);
    const unsigned long long above = lane < 63 ? m >> (lane + 1) : 0ull;
    const uint32_t len = above ? (uint32_t)__ffsll((long long)above) : (uint32_t)(64 - lane);
    const uint32_t sxy = viso_wave_scan(oxy), sz = viso_wave_scan(oz);      // inclusive prefixes
    const int last = lane + (int)len - 1;
    const uint32_t rxy = (uint32_t)__shfl((int)sxy, last) - sxy + oxy;      // the run's sums, in its head lane
    const uint32_t rz = (uint32_t)__shfl((int)sz, last) - sz + oz;
    const bool ins = head && key != MAP_EMPTY;
    bool claimed = false;
    if (ins) map_insert(a.t, key, len, rxy & 0xffffu, rxy >> 16, rz, &claimed);
    map_count_wave(a.t, blockIdx.x + blockIdx.y, lane, point, ins, oor, claimed);
}

__global__ __launch_bounds__(256) void map_add_entries_kernel(MapTable t, const viso_map_entry* e, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const bool on = i < n;
    bool claimed = false;
    if (on) {
        const viso_map_entry v = e[i];
        map_insert(t, map_key(v.k[0], v.k[1], v.k[2]), v.count, v.sum[0], v.sum[1], v.sum[2], &claimed);
        atomicAdd(t.stats + (size_t)(blockIdx.x & (MAP_STAT_SETS - 1)) * MAP_STAT_WORDS + MAP_ST_POINTS, (unsigned long long)v.count);
    }
    map_count_wave(t, blockIdx.x, threadIdx.x & 63, false, on, false, claimed);
}

__global__ __launch_bounds__(256) void map_compact_kernel(MapTable t, uint32_t min_count, viso_map_entry* out, unsigned long long out_cap) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;   // the grid covers the slots exactly (at least 1024 of them)
    const int lane = threadIdx.x & 63;
    const unsigned long long key = t.keys[slot];
    const uint32_t c = t.cnt[slot];
    const bool take = key != MAP_EMPTY && c >= min_count;
    const unsigned long long m = __ballot(take);
    if (!m) return;   // the whole wave
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(t.words + MAP_W_OUT, (unsigned long long)__popcll(m));
    base = __shfl(base, 0);
    const unsigned long long at = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    if (take && out && at < out_cap) {
        viso_map_entry v;
        v.k[0] = (int)((key >> 42) & 0x1fffffu) - MAP_BIAS;
        v.k[1] = (int)((key >> 21) & 0x1fffffu) - MAP_BIAS;
        v.k[2] = (int)(key & 0x1fffffu) - MAP_BIAS;
        v.count = c;
        v.sum[0] = t.sums[3 * (size_t)slot + 0]; v.sum[1] = t.sums[3 * (size_t)slot + 1]; v.sum[2] = t.sums[3 * (size_t)slot + 2];
        out[at] = v;
    }
}

__global__ __launch_bounds__(256) void map_clear_kernel(MapTable t) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    t.keys[slot] = MAP_EMPTY;
    t.cnt[slot] = 0u;
    t.sums[3 * (size_t)slot + 0] = 0ull; t.sums[3 * (size_t)slot + 1] = 0ull; t.sums[3 * (size_t)slot + 2] = 0ull;
    for (uint32_t w = slot; w < MAP_STAT_SETS * MAP_STAT_WORDS; w += t.mask + 1u) t.stats[w] = 0ull;   // (the smallest table has fewer slots)
    if (slot < 2) t.words[slot] = 0ull;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct viso_map {
    viso_ctx* ctx; unsigned long long ctx_serial; int device;
    viso_map_params p; double s;
    MapTable t; void* block;                 // one allocation: keys | sums | cnt | stats | words
    bool overflowed;
    int16_t* d_disp; size_t d_disp_bytes;    // staging of viso_map_fuse's host map (grow-only)
    double* d_pose; size_t d_pose_bytes;     // the poses of a call (grow-only)
    std::mutex mu;
};

static std::mutex g_map_mu;
static std::unordered_set<const viso_map*> g_maps;

static bool map_known(const viso_map* m) {
    std::lock_guard<std::mutex> lk(g_map_mu);
    return m && g_maps.count(m) != 0;
}
static bool map_ctx_live(const viso_map* m) { return viso_ctx_live(m->ctx) && m->ctx->serial == m->ctx_serial; }

// a live map whose context is alive, its device current; else the error text and code
static int map_enter(const char* where, viso_map* m) {
    if (!map_known(m)) { viso_set_error("%s: not a live map handle", where); return VISO_ERR_ARG; }
    if (!map_ctx_live(m)) { viso_set_error("%s: the map's context has been destroyed", where); return VISO_ERR_ARG; }
    HIP_TRY(hipSetDevice(m->device));
    return VISO_OK;
}

static bool map_params_ok(const viso_map_params* p) {
    return p && std::isfinite(p->voxel) && p->voxel > 0.0 && p->min_disp16 >= 1 && p->capacity_log2 >= 10 && p->capacity_log2 <= 28;
}

static bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

extern "C" void viso_map_params_default(viso_map_params* p) {
    if (!p) return;
    p->voxel = 0.2; p->min_disp16 = 16; p->capacity_log2 = 24;
}

static int map_launch_clear(viso_map* m) {
    hipLaunchKernelGGL(map_clear_kernel, dim3((m->t.mask + 1u) / 256u), dim3(256), 0, m->ctx->stream, m->t);
    HIP_TRY(hipGetLastError());
    m->overflowed = false;
    return VISO_OK;
}

extern "C" int viso_map_create(viso_ctx* ctx_or_null, const viso_map_params* params, viso_map** out) {
    if (out) *out = nullptr;
    if (!out || !map_params_ok(params)) {
        viso_set_error("viso_map_create: bad argument (a finite voxel > 0, min_disp16 >= 1, capacity_log2 in 10..28, a non-null output)");
        return VISO_ERR_ARG;
    }
    if (ctx_or_null && !viso_ctx_live(ctx_or_null)) { viso_set_error("viso_map_create: not a live context handle"); return VISO_ERR_ARG; }
    viso_ctx* c = ctx_or_null ? ctx_or_null : viso_default_ctx();
    if (!c) return VISO_ERR_HIP;
    HIP_TRY(hipSetDevice(c->device));
    const size_t slots = (size_t)1 << params->capacity_log2;
    const size_t b_keys = 8 * slots, b_sums = 24 * slots, b_cnt = 4 * slots, b_stats = 8 * MAP_STAT_SETS * MAP_STAT_WORDS;
    const size_t bytes = b_keys + b_sums + b_cnt + b_stats + 256;
    void* block = nullptr;
    if (hipMalloc(&block, bytes) != hipSuccess) {
        (void)hipGetLastError();
        viso_set_error("viso_map_create: cannot allocate the %zu-byte table of 2^%d slots", bytes, (int)params->capacity_log2);
        return VISO_ERR_NOMEM;
    }
    viso_map* m = new viso_map();
    m->ctx = c; m->ctx_serial = c->serial; m->device = c->device;
    m->p = *params; m->s = params->voxel / 1024.0;
    m->block = block;
    char* at = static_cast<char*>(block);
    m->t.keys = reinterpret_cast<unsigned long long*>(at); at += b_keys;
    m->t.sums = reinterpret_cast<unsigned long long*>(at); at += b_sums;
    m->t.cnt = reinterpret_cast<uint32_t*>(at); at += b_cnt;
    m->t.stats = reinterpret_cast<unsigned long long*>(at); at += b_stats;
    m->t.words = reinterpret_cast<unsigned long long*>(at);
    m->t.mask = (uint32_t)(slots - 1);
    m->overflowed = false;
    m->d_disp = nullptr; m->d_disp_bytes = 0; m->d_pose = nullptr; m->d_pose_bytes = 0;
    const int r = map_launch_clear(m);
    if (r < 0) { (void)hipFree(block); delete m; return r; }
    { std::lock_guard<std::mutex> lk(g_map_mu); g_maps.insert(m); }
    *out = m;
    return VISO_OK;
}

extern "C" int viso_map_destroy(viso_map* m) {
    if (!m) return VISO_OK;
    {
        std::lock_guard<std::mutex> lk(g_map_mu);
        if (!g_maps.erase(m)) { viso_set_error("viso_map_destroy: not a live map handle"); return VISO_ERR_ARG; }
    }
    hipError_t first = hipSetDevice(m->device);
    auto note = [&](hipError_t e) { if (e != hipSuccess && first == hipSuccess) first = e; };
    if (map_ctx_live(m)) note(hipStreamSynchronize(m->ctx->stream));   // a destroyed context has waited for its streams itself
    note(hipFree(m->block));
    if (m->d_disp) note(hipFree(m->d_disp));
    if (m->d_pose) note(hipFree(m->d_pose));
    delete m;
    if (first != hipSuccess) { viso_set_error("viso_map_destroy: %s", hipGetErrorString(first)); return VISO_ERR_HIP; }
    return VISO_OK;
}

extern "C" int viso_map_clear(viso_map* m) {
    int r;
    if ((r = map_enter("viso_map_clear", m)) < 0) return r;
    std::lock_guard<std::mutex> lk(m->mu);
    return map_launch_clear(m);
}

static int map_refuse_overflowed(const char* where) {
    viso_set_error("%s: the map has overflowed (points were dropped; which ones depends on scheduling): viso_map_clear it, or use a larger capacity_log2", where);
    return VISO_ERR_NOMEM;
}

template <class T>
static int map_grow(const char* where, T** p, size_t* have, size_t bytes, hipStream_t s) {
    if (*have >= bytes) return VISO_OK;
    HIP_TRY(hipStreamSynchronize(s));   // nothing in flight reads the old block
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr; *have = 0;
    if (hipMalloc((void**)p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        viso_set_error("%s: cannot allocate %zu bytes of staging", where, bytes);
        return VISO_ERR_NOMEM;
    }
    *have = bytes;
    return VISO_OK;
}

// behind a call's launches: waits for them and turns dropped points into the overflow mark
static int map_finish(const char* where, viso_map* m) {
    unsigned long long dropped = 0;
    hipStream_t s = m->ctx->stream;
    HIP_TRY(hipMemcpyAsync(&dropped, m->t.words + MAP_W_DROPPED, sizeof(dropped), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (dropped) {
        m->overflowed = true;
        viso_set_error("%s: the table of 2^%d slots is full: %llu points found no slot (viso_map_clear, or a larger capacity_log2)", where,
                       (int)m->p.capacity_log2, dropped);
        return VISO_ERR_NOMEM;
    }
    return VISO_OK;
}

// the map is entered and locked; disp on the map's device
static int map_fuse_device(const char* where, viso_map* m, const int16_t* disp, size_t mfs, int rows, int cols, int n_frames, double f,
                           double cu, double cv, double base, const double* poses) {
    if (m->overflowed) return map_refuse_overflowed(where);
    hipStream_t s = m->ctx->stream;
    int r;
    std::vector<double> rows12;
    if (poses) {
        rows12.resize((size_t)n_frames * 12);
        for (int k = 0; k < n_frames; ++k) std::copy(poses + (size_t)k * 16, poses + (size_t)k * 16 + 12, rows12.begin() + (size_t)k * 12);
        if ((r = map_grow(where, &m->d_pose, &m->d_pose_bytes, rows12.size() * sizeof(double), s)) < 0) return r;
        HIP_TRY(hipMemcpyAsync(m->d_pose, rows12.data(), rows12.size() * sizeof(double), hipMemcpyHostToDevice, s));
    }
    FuseArgs a;
    a.mfs = mfs; a.rows = rows; a.cols = cols; a.min_disp16 = m->p.min_disp16; a._pad = 0;
    a.f = f; a.cu = cu; a.cv = cv; a.base = base; a.s = m->s; a.t = m->t;
    const size_t px = (size_t)rows * cols;
    for (int f0 = 0; f0 < n_frames; f0 += MAP_GROUP) {
        const int nf = n_frames - f0 < MAP_GROUP ? n_frames - f0 : MAP_GROUP;
        a.disp = disp + (size_t)f0 * mfs;
        a.poses = poses ? m->d_pose + (size_t)f0 * 12 : nullptr;
        hipLaunchKernelGGL(map_fuse_kernel, dim3((unsigned)((px + 255) / 256), (unsigned)nf), dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
    }
    return map_finish(where, m);   // (also keeps rows12 alive until the copy has read it)
}

int map_fuse_resident(const char* where, viso_map* m, viso_ctx* c, const int16_t* disp, size_t mfs, int rows, int cols, int n_frames,
                      double f, double cu, double cv, double base, const double* poses) {
    if (!map_known(m)) { viso_set_error("%s: not a live map handle", where); return VISO_ERR_ARG; }
    if (poses && !all_finite(poses, (size_t)n_frames * 16)) { viso_set_error("%s: a pose has an entry that is not finite", where); return VISO_ERR_ARG; }
    if (!all_finite(&f, 1) || !all_finite(&cu, 1) || !all_finite(&cv, 1) || !all_finite(&base, 1)) {
        viso_set_error("%s: the calibration (f, cu, cv, base) must be finite", where);
        return VISO_ERR_ARG;
    }
    if ((long long)rows * cols > MAP_MAX_PIXELS) { viso_set_error("%s: a %d x %d map is beyond this build (2^31 - 1 pixels)", where, rows, cols); return VISO_ERR_UNSUPPORTED; }
    int r;
    if ((r = map_enter(where, m)) < 0) return r;
    if (m->ctx != c) { viso_set_error("%s: the map and the batch must share a context", where); return VISO_ERR_ARG; }
    std::lock_guard<std::mutex> lk(m->mu);
    return map_fuse_device(where, m, disp, mfs, rows, cols, n_frames, f, cu, cv, base, poses);
}

extern "C" int viso_map_fuse(viso_map* m, const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_or_null) {
    const char* where = "viso_map_fuse";
    if (!map_known(m)) { viso_set_error("%s: not a live map handle", where); return VISO_ERR_ARG; }
    if (!disp || !param || rows <= 0 || cols <= 0) { viso_set_error("%s: bad argument (non-null map and calibration, sizes > 0)", where); return VISO_ERR_ARG; }
    if (pose_or_null && !all_finite(pose_or_null, 16)) { viso_set_error("%s: the pose has an entry that is not finite", where); return VISO_ERR_ARG; }
    if (!std::isfinite(param->f) || !std::isfinite(param->cu) || !std::isfinite(param->cv) || !std::isfinite(param->base)) {
        viso_set_error("%s: the calibration (f, cu, cv, base) must be finite", where);
        return VISO_ERR_ARG;
    }
    if ((long long)rows * cols > MAP_MAX_PIXELS) { viso_set_error("%s: a %d x %d map is beyond this build (2^31 - 1 pixels)", where, rows, cols); return VISO_ERR_UNSUPPORTED; }
    int r;
    if ((r = map_enter(where, m)) < 0) return r;
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->overflowed) return map_refuse_overflowed(where);
    const size_t px = (size_t)rows * cols;
    hipStream_t s = m->ctx->stream;
    if ((r = map_grow(where, &m->d_disp, &m->d_disp_bytes, px * sizeof(int16_t), s)) < 0) return r;
    HIP_TRY(hipMemcpyAsync(m->d_disp, disp, px * sizeof(int16_t), hipMemcpyHostToDevice, s));
    return map_fuse_device(where, m, m->d_disp, px, rows, cols, 1, param->f, param->cu, param->cv, param->base, pose_or_null);
}

extern "C" int viso_map_add_entries(viso_map* m, const viso_map_entry* entries, size_t n) {
    const char* where = "viso_map_add_entries";
    if (!map_known(m)) { viso_set_error("%s: not a live map handle", where); return VISO_ERR_ARG; }
    if (n && !entries) { viso_set_error("%s: bad argument (null entries)", where); return VISO_ERR_ARG; }
    for (size_t i = 0; i < n; ++i) {
        const viso_map_entry& e = entries[i];
        bool ok = e.count >= 1;
        for (int k = 0; k < 3; ++k) ok = ok && e.k[k] >= -MAP_BIAS && e.k[k] < MAP_BIAS && e.sum[k] <= 1023ull * e.count;
        if (!ok) { viso_set_error("%s: entry %zu is not a voxel of a map (k in -2^20 .. 2^20 - 1, count >= 1, sum <= 1023 count)", where, i); return VISO_ERR_ARG; }
    }
    int r;
    if ((r = map_enter(where, m)) < 0) return r;
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->overflowed) return map_refuse_overflowed(where);
    if (!n) return VISO_OK;
    hipStream_t s = m->ctx->stream;
    viso_map_entry* d = nullptr;
    if (hipMalloc((void**)&d, n * sizeof(viso_map_entry)) != hipSuccess) {
        (void)hipGetLastError();
        viso_set_error("%s: cannot allocate %zu bytes for the entries", where, n * sizeof(viso_map_entry));
        return VISO_ERR_NOMEM;
    }
    hipError_t e = hipMemcpyAsync(d, entries, n * sizeof(viso_map_entry), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(map_add_entries_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, m->t, d, (unsigned long long)n);
        e = hipGetLastError();
    }
    r = e == hipSuccess ? map_finish(where, m) : VISO_OK;
    if (e != hipSuccess) (void)hipStreamSynchronize(s);
    (void)hipFree(d);
    HIP_TRY(e);
    return r;
}

// the compaction's pass: the number of voxels with count >= min_count, written to `out` (up to out_cap of them) when it is set
static int map_compact(viso_map* m, uint32_t min_count, viso_map_entry* out, size_t out_cap, unsigned long long* n) {
    hipStream_t s = m->ctx->stream;
    HIP_TRY(hipMemsetAsync(m->t.words + MAP_W_OUT, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(map_compact_kernel, dim3((m->t.mask + 1u) / 256u), dim3(256), 0, s, m->t, min_count, out, (unsigned long long)out_cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(n, m->t.words + MAP_W_OUT, sizeof(*n), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VISO_OK;
}

extern "C" int viso_map_count(viso_map* m, uint32_t min_count, size_t* n) {
    const char* where = "viso_map_count";
    if (!map_known(m)) { viso_set_error("%s: not a live map handle", where); return VISO_ERR_ARG; }
    if (!n || min_count < 1) { viso_set_error("%s: bad argument (min_count >= 1, a non-null output)", where); return VISO_ERR_ARG; }
    int r;
    if ((r = map_enter(where, m)) < 0) return r;
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->overflowed) return map_refuse_overflowed(where);
    unsigned long long c = 0;
    if ((r = map_compact(m, min_count, nullptr, 0, &c)) < 0) return r;
    *n = (size_t)c;
    return VISO_OK;
}

static inline unsigned long long entry_key(const viso_map_entry& e) {
    return ((unsigned long long)(uint32_t)(e.k[0] + MAP_BIAS) << 42) | ((unsigned long long)(uint32_t)(e.k[1] + MAP_BIAS) << 21) |
           (unsigned long long)(uint32_t)(e.k[2] + MAP_BIAS);
}

extern "C" int viso_map_get(viso_map* m, uint32_t min_count, viso_map_entry* entries_out, size_t n_cap, size_t* n) {
    const char* where = "viso_map_get";
    if (!map_known(m)) { viso_set_error("%s: not a live map handle", where); return VISO_ERR_ARG; }
    if (!n || min_count < 1 || (n_cap && !entries_out)) { viso_set_error("%s: bad argument (min_count >= 1, non-null outputs)", where); return VISO_ERR_ARG; }
    int r;
    if ((r = map_enter(where, m)) < 0) return r;
    std::lock_guard<std::mutex> lk(m->mu);
    if (m->overflowed) return map_refuse_overflowed(where);
    unsigned long long c = 0;
    if ((r = map_compact(m, min_count, nullptr, 0, &c)) < 0) return r;
    *n = (size_t)c;
    if (c > n_cap) { viso_set_error("%s: %llu voxels do not fit the %zu entries given", where, c, n_cap); return VISO_ERR_ARG; }
    if (!c) return VISO_OK;
    viso_map_entry* d = nullptr;
    if (hipMalloc((void**)&d, (size_t)c * sizeof(viso_map_entry)) != hipSuccess) {
        (void)hipGetLastError();
        viso_set_error("%s: cannot allocate %zu bytes for the entries", where, (size_t)c * sizeof(viso_map_entry));
        return VISO_ERR_NOMEM;
    }
    unsigned long long c2 = 0;
    r = map_compact(m, min_count, d, (size_t)c, &c2);
    hipError_t e = hipSuccess;
    if (r >= 0) e = hipMemcpy(entries_out, d, (size_t)c * sizeof(viso_map_entry), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (r < 0) return r;
    HIP_TRY(e);
    if (c2 != c) { viso_set_error("%s: the table changed between the two passes", where); return VISO_ERR_HIP; }   // (the map's lock rules it out)
    std::sort(entries_out, entries_out + c, [](const viso_map_entry& x, const viso_map_entry& y) { return entry_key(x) < entry_key(y); });
    return VISO_OK;
}

extern "C" int viso_map_stats(viso_map* m, viso_map_counters* out) {
    const char* where = "viso_map_stats";
    if (!map_known(m)) { viso_set_error("%s: not a live map handle", where); return VISO_ERR_ARG; }
    if (!out) { viso_set_error("%s: bad argument (a non-null output)", where); return VISO_ERR_ARG; }
    int r;
    if ((r = map_enter(where, m)) < 0) return r;
    std::lock_guard<std::mutex> lk(m->mu);
    std::vector<unsigned long long> h((size_t)MAP_STAT_SETS * MAP_STAT_WORDS + 2);
    hipStream_t s = m->ctx->stream;
    HIP_TRY(hipMemcpyAsync(h.data(), m->t.stats, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));   // stats | words: adjacent
    HIP_TRY(hipStreamSynchronize(s));
    viso_map_counters c = {0, 0, 0, 0, 0};
    for (int k = 0; k < MAP_STAT_SETS; ++k) {
        const unsigned long long* st = h.data() + (size_t)k * MAP_STAT_WORDS;
        c.n_points += st[MAP_ST_POINTS]; c.n_inserts += st[MAP_ST_INSERTS]; c.n_out_of_range += st[MAP_ST_OOR]; c.n_occupied += st[MAP_ST_OCC];
    }
    c.n_dropped = h[(size_t)MAP_STAT_SETS * MAP_STAT_WORDS + MAP_W_DROPPED];
    *out = c;
    return VISO_OK;
}

extern "C" int viso_map_entry_centroid(const viso_map_entry* entry, double voxel, float out[3]) {
    if (!entry || !out || entry->count < 1 || !(std::isfinite(voxel) && voxel > 0.0)) {
        viso_set_error("viso_map_entry_centroid: bad argument (non-null entry and output, count >= 1, a finite voxel > 0)");
        return VISO_ERR_ARG;
    }
    const double s = voxel / 1024.0;
    for (int i = 0; i < 3; ++i) {
        const double base = (double)((long long)entry->k[i] * 1024);
        const double mean = (double)entry->sum[i] / (double)entry->count;
        out[i] = (float)(((base + mean) + 0.5) * s);
    }
    return VISO_OK;
}
