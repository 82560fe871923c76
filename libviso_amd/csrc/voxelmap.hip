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
// What every table of voxels shares is not here: the key, the probes, a pixel's point, the runs of a wave, the counters (256 sets on
// cache lines of their own, one atomic per wave and counter, summed on the host), the list positions and the kernels that list,
// clear, add entries to and evict slots (templates over a kind's payload, instantiated here over MapPayload) are voxel_hash.h; the
// handles, the life of a table, the staging and the group loop of a fuse, the scaffold of add_entries, the two passes of the
// getters, the eviction and the statistics' read-back are voxel_host.h.  This file keeps the table's payload, the fuse kernel and
// its insert, the parameter and entry checks and the order of the entries.
#include "common.h"
#include "wave.h"
#include "voxel_host.h"

#include <cmath>

struct MapTable {
    VoxelTable head;
    uint32_t* cnt; unsigned long long* sums;   // [slots], [slots][3]
};

// count points with offset sums sx, sy, sz into the voxel `key`
__device__ __forceinline__ void map_insert(const MapTable& t, unsigned long long key, uint32_t count, unsigned long long sx,
                                           unsigned long long sy, unsigned long long sz, bool* claimed) {
    uint32_t slot;
    if (voxel_probe(t.head.keys, t.head.mask, key, &slot, claimed)) {
        atomicAdd(t.cnt + slot, count);
        atomicAdd(t.sums + 3 * (size_t)slot + 0, sx);
        atomicAdd(t.sums + 3 * (size_t)slot + 1, sy);
        atomicAdd(t.sums + 3 * (size_t)slot + 2, sz);
    } else {
        atomicAdd(t.head.words + VOXEL_W_DROPPED, (unsigned long long)count);
    }
}

// the totals of a wave's four flags; every lane of the wave calls
__device__ __forceinline__ void map_count_wave(const MapTable& t, unsigned block, int lane, bool points, bool inserts, bool oor, bool occ) {
    voxel_count_wave(t.head, block, lane, __popcll(__ballot(points)), __popcll(__ballot(inserts)), __popcll(__ballot(oor)), __popcll(__ballot(occ)));
}

struct FuseArgs {
    VoxelFuseArgs v;
    double s;
    MapTable t;
};

__global__ __launch_bounds__(256) void map_fuse_kernel(FuseArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, fr = blockIdx.y;
    unsigned long long key = MAP_EMPTY;
    uint32_t oxy = 0, oz = 0;     // ox | oy << 16: a wave's sums stay below 2^16 a field (64 x 1023)
    bool oor = false;
    double X, Y, Z;
    const bool point = voxel_point(a.v, i, fr, &X, &Y, &Z);
    if (point) {
        if (a.v.poses) {
            const double* T = a.v.poses + (size_t)fr * 12;
            const double p0 = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
            const double p1 = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
            const double p2 = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
            X = p0; Y = p1; Z = p2;
        }
        const double gx = floor(X / a.s), gy = floor(Y / a.s), gz = floor(Z / a.s);
        if (fabs(gx) < MAP_RANGE && fabs(gy) < MAP_RANGE && fabs(gz) < MAP_RANGE) {   // false for a NaN
            const int ix = (int)gx, iy = (int)gy, iz = (int)gz;
            key = voxel_key(ix >> 10, iy >> 10, iz >> 10);
            oxy = (uint32_t)(ix & 1023) | ((uint32_t)(iy & 1023) << 16);
            oz = (uint32_t)(iz & 1023);
        } else {
            oor = true;
        }
    }
    // the runs of equal keys along the wave (lanes without a point: runs of the empty key, which insert nothing)
    bool head;
    uint32_t len;
    voxel_runs(key, lane, &head, &len);
    const uint32_t sxy = viso_wave_scan(oxy), sz = viso_wave_scan(oz);      // inclusive prefixes
    const int last = lane + (int)len - 1;
    const uint32_t rxy = (uint32_t)__shfl((int)sxy, last) - sxy + oxy;      // the run's sums, in its head lane
    const uint32_t rz = (uint32_t)__shfl((int)sz, last) - sz + oz;
    const bool ins = head && key != MAP_EMPTY;
    bool claimed = false;
    if (ins) map_insert(a.t, key, len, rxy & 0xffffu, rxy >> 16, rz, &claimed);
    map_count_wave(a.t, blockIdx.x + blockIdx.y, lane, point, ins, oor, claimed);
}

// what is in a slot, for the shared kernels that list, zero, add to and evict slots (voxel_hash.h, "a kind's payload")
struct MapPayload {
    MapTable t;
    using Entry = viso_map_entry;
    static constexpr int UNITS_STAT = VOXEL_ST_POINTS;   // add_entries: an entry's count to n_points,
    static constexpr bool ENTRY_STAT = true;             // and one insert an entry
    __host__ __device__ __forceinline__ const VoxelTable& head() const { return t.head; }
    __device__ __forceinline__ uint32_t threshold(uint32_t slot) const { return t.cnt[slot]; }
    __device__ __forceinline__ static unsigned long long key(const Entry& v) { return voxel_key(v.k[0], v.k[1], v.k[2]); }
    __device__ __forceinline__ static unsigned long long units(const Entry& v) { return v.count; }
    __device__ __forceinline__ void add(uint32_t slot, const Entry& v) const {
        atomicAdd(t.cnt + slot, v.count);
        for (int i = 0; i < 3; ++i) atomicAdd(t.sums + 3 * (size_t)slot + i, v.sum[i]);
    }
    __device__ __forceinline__ void pack(uint32_t slot, unsigned long long key, uint32_t count, Entry* v) const {
        voxel_unkey(key, v->k);
        v->count = count;
        v->sum[0] = t.sums[3 * (size_t)slot + 0]; v->sum[1] = t.sums[3 * (size_t)slot + 1]; v->sum[2] = t.sums[3 * (size_t)slot + 2];
    }
    __device__ __forceinline__ void zero(uint32_t a) const {
        t.cnt[a] = 0u;
        t.sums[3 * (size_t)a + 0] = 0ull; t.sums[3 * (size_t)a + 1] = 0ull; t.sums[3 * (size_t)a + 2] = 0ull;
    }
    __device__ __forceinline__ void move(uint32_t a, uint32_t b) const {
        t.cnt[b] = t.cnt[a];
        for (int i = 0; i < 3; ++i) t.sums[3 * (size_t)b + i] = t.sums[3 * (size_t)a + i];
        zero(a);
    }
};

// ---- host: what is the voxel map's own; the rest is the shared layer's (voxel_host.h) --------------------------------------------
struct viso_map {
    VoxelHost h;
    viso_map_params p; double s;
    MapTable t;                              // the payload in h's block: sums | cnt
};

static VoxelRegistry g_maps = {{"map", "map", "points", "min_count", "viso_map_clear"}};

static bool map_params_ok(const viso_map_params* p) {
    return p && std::isfinite(p->voxel) && p->voxel > 0.0 && p->min_disp16 >= 1 && p->capacity_log2 >= 10 && p->capacity_log2 <= 28;
}

extern "C" void viso_map_params_default(viso_map_params* p) {
    if (!p) return;
    p->voxel = 0.2; p->min_disp16 = 16; p->capacity_log2 = 24;
}

// the launches the shared layer asks for; m is live by then
static VoxelLaunch map_clear_launch(viso_map* m) {
    return [m](hipStream_t s) { voxel_start_clear(MapPayload{m->t}, s); };
}
static VoxelFuseLaunch map_fuse_launch(viso_map* m) {
    return [m](const VoxelFuseArgs& v, const uint8_t*, dim3 grid, hipStream_t s) {   // (a voxel map fuses no image)
        FuseArgs a;
        a.v = v; a.s = m->s; a.t = m->t;
        hipLaunchKernelGGL(map_fuse_kernel, grid, dim3(256), 0, s, a);
    };
}

extern "C" int viso_map_create(viso_ctx* ctx_or_null, const viso_map_params* params, viso_map** out) {
    if (out) *out = nullptr;
    if (!out || !map_params_ok(params)) {
        viso_set_error("viso_map_create: bad argument (a finite voxel > 0, min_disp16 >= 1, capacity_log2 in 10..28, a non-null output)");
        return VISO_ERR_ARG;
    }
    viso_map* m = new viso_map();
    char* payload;
    int r = voxel_create("viso_map_create", g_maps, ctx_or_null, params->capacity_log2, params->min_disp16, 28, &m->h, &payload);
    if (r >= 0) {
        m->p = *params; m->s = params->voxel / 1024.0;
        m->t.head = m->h.head;
        m->t.sums = reinterpret_cast<unsigned long long*>(payload);
        m->t.cnt = reinterpret_cast<uint32_t*>(payload + 24 * ((size_t)1 << params->capacity_log2));
        r = voxel_open(g_maps, m, &m->h, map_clear_launch(m));
    }
    if (r < 0) { delete m; return r; }
    *out = m;
    return VISO_OK;
}

extern "C" int viso_map_destroy(viso_map* m) {
    if (!m) return VISO_OK;
    if (!voxel_unregister("viso_map_destroy", g_maps, m)) return VISO_ERR_ARG;
    const int r = voxel_free("viso_map_destroy", &m->h);
    delete m;
    return r;
}

extern "C" int viso_map_clear(viso_map* m) { return voxel_clear("viso_map_clear", g_maps, m, map_clear_launch(m)); }

int map_fuse_resident(const char* where, viso_map* m, const DispView& v) { return voxel_fuse(where, g_maps, m, v, map_fuse_launch(m)); }

extern "C" int viso_map_fuse(viso_map* m, const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_or_null) {
    return voxel_fuse("viso_map_fuse", g_maps, m, disp_view_host(disp, nullptr, rows, cols, param, pose_or_null), map_fuse_launch(m));
}

extern "C" int viso_map_add_entries(viso_map* m, const viso_map_entry* entries, size_t n) {
    const char* where = "viso_map_add_entries";
    if (!voxel_known(g_maps, m)) { viso_set_error("%s: not a live map handle", where); return VISO_ERR_ARG; }
    if (n && !entries) { viso_set_error("%s: bad argument (null entries)", where); return VISO_ERR_ARG; }
    for (size_t i = 0; i < n; ++i) {
        const viso_map_entry& e = entries[i];
        bool ok = e.count >= 1;
        for (int k = 0; k < 3; ++k) ok = ok && e.k[k] >= -MAP_BIAS && e.k[k] < MAP_BIAS && e.sum[k] <= 1023ull * e.count;
        if (!ok) { viso_set_error("%s: entry %zu is not a voxel of a map (k in -2^20 .. 2^20 - 1, count >= 1, sum <= 1023 count)", where, i); return VISO_ERR_ARG; }
    }
    return voxel_add_entries(where, g_maps, m, entries, n, MapPayload{m->t});
}

static inline bool voxel_item_less(const viso_map_entry& x, const viso_map_entry& y) {
    return voxel_key(x.k[0], x.k[1], x.k[2]) < voxel_key(y.k[0], y.k[1], y.k[2]);
}

// the count or the sorted list of the voxels with count >= min_count
static int map_extract(const char* where, viso_map* m, uint32_t min_count, const VoxelList<viso_map_entry>& list) {
    if (!voxel_known(g_maps, m)) { viso_set_error("%s: not a live map handle", where); return VISO_ERR_ARG; }
    return voxel_entries(where, g_maps, m, min_count, list, MapPayload{m->t});
}
extern "C" int viso_map_count(viso_map* m, uint32_t min_count, size_t* n) { return map_extract("viso_map_count", m, min_count, {true, nullptr, 0, n}); }
extern "C" int viso_map_get(viso_map* m, uint32_t min_count, viso_map_entry* entries_out, size_t n_cap, size_t* n) {
    return map_extract("viso_map_get", m, min_count, {false, entries_out, n_cap, n});
}

static int map_evict(const char* where, viso_map* m, const viso_voxel_box* keep, const VoxelList<viso_map_entry>& list) {
    if (!voxel_known(g_maps, m)) { viso_set_error("%s: not a live map handle", where); return VISO_ERR_ARG; }
    return voxel_evict(where, g_maps, m, keep, list, MapPayload{m->t});
}
extern "C" int viso_map_evict_count(viso_map* m, const viso_voxel_box* keep, size_t* n) {
    return map_evict("viso_map_evict_count", m, keep, {true, nullptr, 0, n});
}
extern "C" int viso_map_evict(viso_map* m, const viso_voxel_box* keep, viso_map_entry* evicted_out, size_t n_cap, size_t* n) {
    return map_evict("viso_map_evict", m, keep, {false, evicted_out, n_cap, n});
}

extern "C" int viso_map_stats(viso_map* m, viso_map_counters* out) {
    unsigned long long sums[4], dropped;
    const int r = voxel_stats("viso_map_stats", g_maps, m, out, sums, &dropped);
    if (r < 0) return r;
    out->n_points = sums[VOXEL_ST_POINTS]; out->n_inserts = sums[VOXEL_ST_UPDATES]; out->n_out_of_range = sums[VOXEL_ST_OOR];
    out->n_occupied = sums[VOXEL_ST_OCC]; out->n_dropped = dropped;
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
