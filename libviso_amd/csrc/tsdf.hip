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
//   tsdf_add_entries_kernel  one thread per entry through the same probe.
//   tsdf_compact_kernel      one thread per slot: the slots with weight >= min_weight to a dense list, one atomic per wave for the
//                            list positions (out == null: only their number).
//   tsdf_crossings_kernel    one thread per slot, three read-only probes for the neighbours at +1 on every axis; the same two passes.
//   tsdf_mesh_kernel         one thread per slot, seven read-only probes for the other corners of the voxel's cell: the sign-changing
//                            edges the voxel owns as vertices, and the triangles of the cell's six tetrahedra as references to
//                            them; two lists, one atomic per wave and list; the same two passes.
//   tsdf_clear_kernel        one thread per slot.
// The statistics are 256 sets of counters on cache lines of their own (a wave adds its totals once, at its end), summed on the host.
#include "common.h"
#include "voxel_hash.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <type_traits>
#include <unordered_set>
#include <vector>

#define TSDF_STAT_SETS 256
#define TSDF_STAT_WORDS 16              // 128 bytes a set
#define TSDF_ST_POINTS 0
#define TSDF_ST_UPDATES 1
#define TSDF_ST_OOR 2
#define TSDF_ST_OCC 3
#define TSDF_W_OUT 0                    // words: an extraction's list length
#define TSDF_W_DROPPED 1                //        updates that found no slot
#define TSDF_MAX_PIXELS 0x7fffffffll
#define TSDF_GROUP 16384                // frames along a grid's y

struct TsdfTable {
    unsigned long long* keys; unsigned long long* sum; uint32_t* weight;
    unsigned long long* stats;   // [TSDF_STAT_SETS][TSDF_STAT_WORDS]
    unsigned long long* words;   // TSDF_W_*
    uint32_t mask;               // slots - 1
};

// weight updates with the sum of q `sum` into the voxel `key`
__device__ __forceinline__ void tsdf_insert(const TsdfTable& t, unsigned long long key, uint32_t weight, long long sum, bool* claimed) {
    uint32_t slot;
    if (voxel_probe(t.keys, t.mask, key, &slot, claimed)) {
        atomicAdd(t.weight + slot, weight);
        atomicAdd(t.sum + slot, (unsigned long long)sum);
    } else {
        atomicAdd(t.words + TSDF_W_DROPPED, (unsigned long long)weight);
    }
}

__device__ __forceinline__ void tsdf_count_wave(const TsdfTable& t, unsigned block, int lane, unsigned long long points,
                                                unsigned long long updates, unsigned long long oor, unsigned long long occ) {
    if (lane == 0) {
        unsigned long long* st = t.stats + (size_t)(block & (TSDF_STAT_SETS - 1)) * TSDF_STAT_WORDS;
        if (points) atomicAdd(st + TSDF_ST_POINTS, points);
        if (updates) atomicAdd(st + TSDF_ST_UPDATES, updates);
        if (oor) atomicAdd(st + TSDF_ST_OOR, oor);
        if (occ) atomicAdd(st + TSDF_ST_OCC, occ);
    }
}

struct TsdfFuseArgs {
    const int16_t* disp; size_t mfs;   // frame f's map at disp + f * mfs
    const double* poses;               // [frames][12] on the device, or null: no transform
    int rows, cols, min_disp16, trunc;
    double f, cu, cv, base, s, h;
    TsdfTable t;
};

__global__ __launch_bounds__(256) void tsdf_fuse_kernel(TsdfFuseArgs a) {
    const size_t px = (size_t)a.rows * a.cols, i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, fr = blockIdx.y;
    bool point = false;
    double X = 0.0, Y = 0.0, Z = 1.0;
    if (i < px) {
        const int d16 = a.disp[(size_t)fr * a.mfs + i];
        if (d16 != VISO_DISP_INVALID && d16 >= a.min_disp16) {
            point = true;
            const int y = (int)(i / (size_t)a.cols), x = (int)(i - (size_t)y * a.cols);
            const double d = (double)d16 / 16.0;
            X = a.base * ((double)x - a.cu) / d;      // the operand order of points_kernel (speckle.hip)
            Y = a.base * ((double)y - a.cv) / d;
            Z = a.f * a.base / d;
        }
    }
    const unsigned long long pm = __ballot(point);
    if (!pm) return;   // the whole wave
    // Without a pose the identity: ((1 a + 0 b) + 0 c) + 0 = a and (0 a + 0 b) + 1 (c - 0) = c for finite a, b, c, up to the sign
    // of a zero, which neither floor(. / s) nor Z - zc keeps.
    double T0 = 1.0, T1 = 0.0, T2 = 0.0, T3 = 0.0, T4 = 0.0, T5 = 1.0, T6 = 0.0, T7 = 0.0, T8 = 0.0, T9 = 0.0, T10 = 1.0, T11 = 0.0;
    if (a.poses) {
        const double* T = a.poses + (size_t)fr * 12;
        T0 = T[0]; T1 = T[1]; T2 = T[2]; T3 = T[3]; T4 = T[4]; T5 = T[5]; T6 = T[6]; T7 = T[7]; T8 = T[8]; T9 = T[9]; T10 = T[10]; T11 = T[11];
    }
    const int lim = a.trunc * 1024;
    const double dlim = (double)lim;
    unsigned long long prev = MAP_EMPTY;            // the voxel of the pixel's previous inserted sample
    unsigned long long n_upd = 0, n_oor = 0, n_occ = 0;
    for (int j = -2 * a.trunc; j <= 2 * a.trunc; ++j) {   // the same j in every lane
        unsigned long long key = MAP_EMPTY;
        uint32_t qb = 0;                            // q + T 1024
        bool oor = false;
        if (point) {
            const double zj = Z + (double)j * a.h;
            if (zj > 0.0) {
                const double r = zj / Z;
                const double c0 = X * r, c1 = Y * r;
                const double gx = floor((((T0 * c0 + T1 * c1) + T2 * zj) + T3) / a.s);
                const double gy = floor((((T4 * c0 + T5 * c1) + T6 * zj) + T7) / a.s);
                const double gz = floor((((T8 * c0 + T9 * c1) + T10 * zj) + T11) / a.s);
                if (fabs(gx) < MAP_RANGE && fabs(gy) < MAP_RANGE && fabs(gz) < MAP_RANGE) {   // false for a NaN
                    const int kx = (int)gx >> 10, ky = (int)gy >> 10, kz = (int)gz >> 10;
                    const unsigned long long k = map_key(kx, ky, kz);
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
        const unsigned long long kl = __shfl_up(key, 1);
        const bool head = lane == 0 || key != kl;
        const unsigned long long m = __ballot(head);
        const unsigned long long above = lane < 63 ? m >> (lane + 1) : 0ull;
        const uint32_t len = above ? (uint32_t)__ffsll((long long)above) : (uint32_t)(64 - lane);
        const uint32_t sq = viso_wave_scan(qb);                                   // inclusive prefix
        const uint32_t rq = (uint32_t)__shfl((int)sq, lane + (int)len - 1) - sq + qb;   // the run's sum, in its head lane
        bool claimed = false;
        if (head && key != MAP_EMPTY) tsdf_insert(a.t, key, len, (long long)rq - (long long)len * lim, &claimed);
        n_occ += __popcll(__ballot(claimed));
    }
    tsdf_count_wave(a.t, blockIdx.x + blockIdx.y, lane, __popcll(pm), n_upd, n_oor, n_occ);
}

__device__ __forceinline__ unsigned long long tsdf_entry_key(const int32_t* k) { return map_key(k[0], k[1], k[2]); }

__global__ __launch_bounds__(256) void tsdf_add_entries_kernel(TsdfTable t, const viso_tsdf_entry* e, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    bool claimed = false;
    unsigned long long w = 0;
    if (i < n) {
        const viso_tsdf_entry v = e[i];
        w = v.weight;
        tsdf_insert(t, tsdf_entry_key(v.k), v.weight, v.sum, &claimed);
        atomicAdd(t.stats + (size_t)(blockIdx.x & (TSDF_STAT_SETS - 1)) * TSDF_STAT_WORDS + TSDF_ST_UPDATES, w);
    }
    tsdf_count_wave(t, blockIdx.x, threadIdx.x & 63, 0, 0, 0, __popcll(__ballot(claimed)));
}

__device__ __forceinline__ void tsdf_unkey(unsigned long long key, int32_t* k) {
    k[0] = (int)((key >> 42) & 0x1fffffu) - MAP_BIAS;
    k[1] = (int)((key >> 21) & 0x1fffffu) - MAP_BIAS;
    k[2] = (int)(key & 0x1fffffu) - MAP_BIAS;
}

__global__ __launch_bounds__(256) void tsdf_compact_kernel(TsdfTable t, uint32_t min_weight, viso_tsdf_entry* out, unsigned long long out_cap) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;   // the grid covers the slots exactly (at least 1024 of them)
    const int lane = threadIdx.x & 63;
    const unsigned long long key = t.keys[slot];
    const uint32_t w = t.weight[slot];
    const bool take = key != MAP_EMPTY && w >= min_weight;
    const unsigned long long m = __ballot(take);
    if (!m) return;   // the whole wave
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(t.words + TSDF_W_OUT, (unsigned long long)__popcll(m));
    base = __shfl(base, 0);
    const unsigned long long at = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    if (take && out && at < out_cap) {
        viso_tsdf_entry v;
        tsdf_unkey(key, v.k);
        v.weight = w;
        v.sum = (long long)t.sum[slot];
        out[at] = v;
    }
}

__global__ __launch_bounds__(256) void tsdf_crossings_kernel(TsdfTable t, uint32_t min_weight, viso_tsdf_crossing* out, unsigned long long out_cap) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;   // the grid covers the slots exactly
    const int lane = threadIdx.x & 63;
    const unsigned long long key = t.keys[slot];
    const uint32_t wa = t.weight[slot];
    const bool take = key != MAP_EMPTY && wa >= min_weight;
    if (!__ballot(take)) return;   // the whole wave
    int32_t k[3] = {0, 0, 0};
    long long sa = 0, sb[3] = {0, 0, 0};
    uint32_t wb[3] = {0, 0, 0};
    bool hit[3] = {false, false, false};
    uint32_t mine = 0;
    if (take) {
        tsdf_unkey(key, k);
        sa = (long long)t.sum[slot];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            if (k[ax] == MAP_BIAS - 1) continue;   // the last voxel of the axis has no neighbour
            uint32_t nb;
            if (!voxel_find(t.keys, t.mask, key + (1ull << (21 * (2 - ax))), &nb)) continue;
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
    if (lane == 0) base = atomicAdd(t.words + TSDF_W_OUT, (unsigned long long)total);
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
#define TSDF_W_TRIS 2                   // words: the triangle list's length (TSDF_W_OUT: the vertex list's)
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
    const unsigned long long key = t.keys[slot];
    const uint32_t wa = t.weight[slot];
    const bool take = key != MAP_EMPTY && wa >= min_weight;
    if (!__ballot(take)) return;   // the whole wave
    int32_t k[3] = {0, 0, 0};
    long long sa = 0, sb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t wb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t usable = 0, neg = 0, hit = 0;   // bit d: the neighbour at d is usable / negative / across a sign change from this voxel
    if (take) {
        tsdf_unkey(key, k);
        sa = (long long)t.sum[slot];
        usable = 1u; neg = sa < 0 ? 1u : 0u;
#pragma unroll
        for (int d = 1; d < 8; ++d) {
            // the last voxel of an axis has no neighbour along it: no key is formed beyond a field
            if (((d & 1) && k[0] == MAP_BIAS - 1) || ((d & 2) && k[1] == MAP_BIAS - 1) || ((d & 4) && k[2] == MAP_BIAS - 1)) continue;
            uint32_t nb;
            if (!voxel_find(t.keys, t.mask, key + ((unsigned long long)(d & 1) << 42) + ((unsigned long long)((d >> 1) & 1) << 21) + (unsigned long long)(d >> 2), &nb)) continue;
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
        if (total & 0xffffu) vbase = atomicAdd(t.words + TSDF_W_OUT, (unsigned long long)(total & 0xffffu));
        if (total >> 16) tbase = atomicAdd(t.words + TSDF_W_TRIS, (unsigned long long)(total >> 16));
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

__global__ __launch_bounds__(256) void tsdf_clear_kernel(TsdfTable t) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    t.keys[slot] = MAP_EMPTY;
    t.weight[slot] = 0u;
    t.sum[slot] = 0ull;
    for (uint32_t w = slot; w < TSDF_STAT_SETS * TSDF_STAT_WORDS; w += t.mask + 1u) t.stats[w] = 0ull;   // (the smallest table has fewer slots)
    if (slot < 2) t.words[slot] = 0ull;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct viso_tsdf {
    viso_ctx* ctx; unsigned long long ctx_serial; int device;
    viso_tsdf_params p; double s, h;
    TsdfTable t; void* block;                // one allocation: keys | sum | weight | stats | words
    bool overflowed;
    int16_t* d_disp; size_t d_disp_bytes;    // staging of viso_tsdf_fuse's host map (grow-only)
    double* d_pose; size_t d_pose_bytes;     // the poses of a call (grow-only)
    std::mutex mu;
};

static std::mutex g_tsdf_mu;
static std::unordered_set<const viso_tsdf*> g_tsdfs;

static bool tsdf_known(const viso_tsdf* t) {
    std::lock_guard<std::mutex> lk(g_tsdf_mu);
    return t && g_tsdfs.count(t) != 0;
}
static bool tsdf_ctx_live(const viso_tsdf* t) { return viso_ctx_live(t->ctx) && t->ctx->serial == t->ctx_serial; }

// a live map whose context is alive, its device current; else the error text and code
static int tsdf_enter(const char* where, viso_tsdf* t) {
    if (!tsdf_known(t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    if (!tsdf_ctx_live(t)) { viso_set_error("%s: the TSDF map's context has been destroyed", where); return VISO_ERR_ARG; }
    HIP_TRY(hipSetDevice(t->device));
    return VISO_OK;
}

static bool tsdf_params_ok(const viso_tsdf_params* p) {
    return p && std::isfinite(p->voxel) && p->voxel > 0.0 && p->trunc_voxels >= 1 && p->trunc_voxels <= 8 && p->min_disp16 >= 1 &&
           p->capacity_log2 >= 10 && p->capacity_log2 <= 28;
}

static bool tsdf_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

extern "C" void viso_tsdf_params_default(viso_tsdf_params* p) {
    if (!p) return;
    p->voxel = 0.2; p->trunc_voxels = 3; p->min_disp16 = 16; p->capacity_log2 = 26;
}

static int tsdf_launch_clear(viso_tsdf* t) {
    hipLaunchKernelGGL(tsdf_clear_kernel, dim3((t->t.mask + 1u) / 256u), dim3(256), 0, t->ctx->stream, t->t);
    HIP_TRY(hipGetLastError());
    t->overflowed = false;
    return VISO_OK;
}

extern "C" int viso_tsdf_create(viso_ctx* ctx_or_null, const viso_tsdf_params* params, viso_tsdf** out) {
    if (out) *out = nullptr;
    if (!out || !tsdf_params_ok(params)) {
        viso_set_error("viso_tsdf_create: bad argument (a finite voxel > 0, trunc_voxels in 1..8, min_disp16 >= 1, capacity_log2 in 10..28, a non-null output)");
        return VISO_ERR_ARG;
    }
    if (ctx_or_null && !viso_ctx_live(ctx_or_null)) { viso_set_error("viso_tsdf_create: not a live context handle"); return VISO_ERR_ARG; }
    viso_ctx* c = ctx_or_null ? ctx_or_null : viso_default_ctx();
    if (!c) return VISO_ERR_HIP;
    HIP_TRY(hipSetDevice(c->device));
    const size_t slots = (size_t)1 << params->capacity_log2;
    const size_t b_keys = 8 * slots, b_sum = 8 * slots, b_weight = 4 * slots, b_stats = 8 * TSDF_STAT_SETS * TSDF_STAT_WORDS;
    const size_t bytes = b_keys + b_sum + b_weight + b_stats + 256;
    void* block = nullptr;
    if (hipMalloc(&block, bytes) != hipSuccess) {
        (void)hipGetLastError();
        viso_set_error("viso_tsdf_create: cannot allocate the %zu-byte table of 2^%d slots", bytes, (int)params->capacity_log2);
        return VISO_ERR_NOMEM;
    }
    viso_tsdf* t = new viso_tsdf();
    t->ctx = c; t->ctx_serial = c->serial; t->device = c->device;
    t->p = *params; t->s = params->voxel / 1024.0; t->h = params->voxel * 0.5;
    t->block = block;
    char* at = static_cast<char*>(block);
    t->t.keys = reinterpret_cast<unsigned long long*>(at); at += b_keys;
    t->t.sum = reinterpret_cast<unsigned long long*>(at); at += b_sum;
    t->t.weight = reinterpret_cast<uint32_t*>(at); at += b_weight;
    t->t.stats = reinterpret_cast<unsigned long long*>(at); at += b_stats;
    t->t.words = reinterpret_cast<unsigned long long*>(at);
    t->t.mask = (uint32_t)(slots - 1);
    t->overflowed = false;
    t->d_disp = nullptr; t->d_disp_bytes = 0; t->d_pose = nullptr; t->d_pose_bytes = 0;
    const int r = tsdf_launch_clear(t);
    if (r < 0) { (void)hipFree(block); delete t; return r; }
    { std::lock_guard<std::mutex> lk(g_tsdf_mu); g_tsdfs.insert(t); }
    *out = t;
    return VISO_OK;
}

extern "C" int viso_tsdf_destroy(viso_tsdf* t) {
    if (!t) return VISO_OK;
    {
        std::lock_guard<std::mutex> lk(g_tsdf_mu);
        if (!g_tsdfs.erase(t)) { viso_set_error("viso_tsdf_destroy: not a live TSDF handle"); return VISO_ERR_ARG; }
    }
    hipError_t first = hipSetDevice(t->device);
    auto note = [&](hipError_t e) { if (e != hipSuccess && first == hipSuccess) first = e; };
    if (tsdf_ctx_live(t)) note(hipStreamSynchronize(t->ctx->stream));   // a destroyed context has waited for its streams itself
    note(hipFree(t->block));
    if (t->d_disp) note(hipFree(t->d_disp));
    if (t->d_pose) note(hipFree(t->d_pose));
    delete t;
    if (first != hipSuccess) { viso_set_error("viso_tsdf_destroy: %s", hipGetErrorString(first)); return VISO_ERR_HIP; }
    return VISO_OK;
}

extern "C" int viso_tsdf_clear(viso_tsdf* t) {
    int r;
    if ((r = tsdf_enter("viso_tsdf_clear", t)) < 0) return r;
    std::lock_guard<std::mutex> lk(t->mu);
    return tsdf_launch_clear(t);
}

static int tsdf_refuse_overflowed(const char* where) {
    viso_set_error("%s: the TSDF map has overflowed (updates were dropped; which ones depends on scheduling): viso_tsdf_clear it, or use a larger capacity_log2", where);
    return VISO_ERR_NOMEM;
}

template <class T>
static int tsdf_grow(const char* where, T** p, size_t* have, size_t bytes, hipStream_t s) {
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

// behind a call's launches: waits for them and turns dropped updates into the overflow mark
static int tsdf_finish(const char* where, viso_tsdf* t) {
    unsigned long long dropped = 0;
    hipStream_t s = t->ctx->stream;
    HIP_TRY(hipMemcpyAsync(&dropped, t->t.words + TSDF_W_DROPPED, sizeof(dropped), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (dropped) {
        t->overflowed = true;
        viso_set_error("%s: the table of 2^%d slots is full: %llu updates found no slot (viso_tsdf_clear, or a larger capacity_log2)", where,
                       (int)t->p.capacity_log2, dropped);
        return VISO_ERR_NOMEM;
    }
    return VISO_OK;
}

// the map is entered and locked; disp on the map's device
static int tsdf_fuse_device(const char* where, viso_tsdf* t, const int16_t* disp, size_t mfs, int rows, int cols, int n_frames, double f,
                            double cu, double cv, double base, const double* poses) {
    if (t->overflowed) return tsdf_refuse_overflowed(where);
    hipStream_t s = t->ctx->stream;
    int r;
    std::vector<double> rows12;
    if (poses) {
        rows12.resize((size_t)n_frames * 12);
        for (int k = 0; k < n_frames; ++k) std::copy(poses + (size_t)k * 16, poses + (size_t)k * 16 + 12, rows12.begin() + (size_t)k * 12);
        if ((r = tsdf_grow(where, &t->d_pose, &t->d_pose_bytes, rows12.size() * sizeof(double), s)) < 0) return r;
        HIP_TRY(hipMemcpyAsync(t->d_pose, rows12.data(), rows12.size() * sizeof(double), hipMemcpyHostToDevice, s));
    }
    TsdfFuseArgs a;
    a.mfs = mfs; a.rows = rows; a.cols = cols; a.min_disp16 = t->p.min_disp16; a.trunc = t->p.trunc_voxels;
    a.f = f; a.cu = cu; a.cv = cv; a.base = base; a.s = t->s; a.h = t->h; a.t = t->t;
    const size_t px = (size_t)rows * cols;
    for (int f0 = 0; f0 < n_frames; f0 += TSDF_GROUP) {
        const int nf = n_frames - f0 < TSDF_GROUP ? n_frames - f0 : TSDF_GROUP;
        a.disp = disp + (size_t)f0 * mfs;
        a.poses = poses ? t->d_pose + (size_t)f0 * 12 : nullptr;
        hipLaunchKernelGGL(tsdf_fuse_kernel, dim3((unsigned)((px + 255) / 256), (unsigned)nf), dim3(256), 0, s, a);
        HIP_TRY(hipGetLastError());
    }
    return tsdf_finish(where, t);   // (also keeps rows12 alive until the copy has read it)
}

static int tsdf_fuse_args(const char* where, int rows, int cols, int n_frames, double f, double cu, double cv, double base, const double* poses) {
    if (poses && !tsdf_finite(poses, (size_t)n_frames * 16)) { viso_set_error("%s: a pose has an entry that is not finite", where); return VISO_ERR_ARG; }
    if (!std::isfinite(f) || !std::isfinite(cu) || !std::isfinite(cv) || !std::isfinite(base)) {
        viso_set_error("%s: the calibration (f, cu, cv, base) must be finite", where);
        return VISO_ERR_ARG;
    }
    if ((long long)rows * cols > TSDF_MAX_PIXELS) { viso_set_error("%s: a %d x %d map is beyond this build (2^31 - 1 pixels)", where, rows, cols); return VISO_ERR_UNSUPPORTED; }
    return VISO_OK;
}

int tsdf_fuse_resident(const char* where, viso_tsdf* t, viso_ctx* c, const int16_t* disp, size_t mfs, int rows, int cols, int n_frames,
                       double f, double cu, double cv, double base, const double* poses) {
    if (!tsdf_known(t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    int r;
    if ((r = tsdf_fuse_args(where, rows, cols, n_frames, f, cu, cv, base, poses)) < 0) return r;
    if ((r = tsdf_enter(where, t)) < 0) return r;
    if (t->ctx != c) { viso_set_error("%s: the TSDF map and the batch must share a context", where); return VISO_ERR_ARG; }
    std::lock_guard<std::mutex> lk(t->mu);
    return tsdf_fuse_device(where, t, disp, mfs, rows, cols, n_frames, f, cu, cv, base, poses);
}

extern "C" int viso_tsdf_fuse(viso_tsdf* t, const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_or_null) {
    const char* where = "viso_tsdf_fuse";
    if (!tsdf_known(t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    if (!disp || !param || rows <= 0 || cols <= 0) { viso_set_error("%s: bad argument (non-null map and calibration, sizes > 0)", where); return VISO_ERR_ARG; }
    int r;
    if ((r = tsdf_fuse_args(where, rows, cols, 1, param->f, param->cu, param->cv, param->base, pose_or_null)) < 0) return r;
    if ((r = tsdf_enter(where, t)) < 0) return r;
    std::lock_guard<std::mutex> lk(t->mu);
    if (t->overflowed) return tsdf_refuse_overflowed(where);
    const size_t px = (size_t)rows * cols;
    hipStream_t s = t->ctx->stream;
    if ((r = tsdf_grow(where, &t->d_disp, &t->d_disp_bytes, px * sizeof(int16_t), s)) < 0) return r;
    HIP_TRY(hipMemcpyAsync(t->d_disp, disp, px * sizeof(int16_t), hipMemcpyHostToDevice, s));
    return tsdf_fuse_device(where, t, t->d_disp, px, rows, cols, 1, param->f, param->cu, param->cv, param->base, pose_or_null);
}

extern "C" int viso_tsdf_add_entries(viso_tsdf* t, const viso_tsdf_entry* entries, size_t n) {
    const char* where = "viso_tsdf_add_entries";
    if (!tsdf_known(t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    if (n && !entries) { viso_set_error("%s: bad argument (null entries)", where); return VISO_ERR_ARG; }
    const long long lim = (long long)t->p.trunc_voxels * 1024;
    for (size_t i = 0; i < n; ++i) {
        const viso_tsdf_entry& e = entries[i];
        bool ok = e.weight >= 1 && e.sum <= lim * (long long)e.weight && e.sum >= -lim * (long long)e.weight;
        for (int k = 0; k < 3; ++k) ok = ok && e.k[k] >= -MAP_BIAS && e.k[k] < MAP_BIAS;
        if (!ok) { viso_set_error("%s: entry %zu is not a voxel of this map (k in -2^20 .. 2^20 - 1, weight >= 1, |sum| <= %lld weight)", where, i, lim); return VISO_ERR_ARG; }
    }
    int r;
    if ((r = tsdf_enter(where, t)) < 0) return r;
    std::lock_guard<std::mutex> lk(t->mu);
    if (t->overflowed) return tsdf_refuse_overflowed(where);
    if (!n) return VISO_OK;
    hipStream_t s = t->ctx->stream;
    viso_tsdf_entry* d = nullptr;
    if (hipMalloc((void**)&d, n * sizeof(viso_tsdf_entry)) != hipSuccess) {
        (void)hipGetLastError();
        viso_set_error("%s: cannot allocate %zu bytes for the entries", where, n * sizeof(viso_tsdf_entry));
        return VISO_ERR_NOMEM;
    }
    hipError_t e = hipMemcpyAsync(d, entries, n * sizeof(viso_tsdf_entry), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(tsdf_add_entries_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t->t, d, (unsigned long long)n);
        e = hipGetLastError();
    }
    r = e == hipSuccess ? tsdf_finish(where, t) : VISO_OK;
    if (e != hipSuccess) (void)hipStreamSynchronize(s);
    (void)hipFree(d);
    HIP_TRY(e);
    return r;
}

// One pass of an extraction (Item = viso_tsdf_entry: the voxels; viso_tsdf_crossing: the crossings): the number of items, written to
// `out` (up to out_cap of them) when it is set
template <class Item>
static int tsdf_pass(viso_tsdf* t, uint32_t min_weight, Item* out, size_t out_cap, unsigned long long* n) {
    hipStream_t s = t->ctx->stream;
    HIP_TRY(hipMemsetAsync(t->t.words + TSDF_W_OUT, 0, sizeof(unsigned long long), s));
    const dim3 grid((t->t.mask + 1u) / 256u);
    if constexpr (std::is_same<Item, viso_tsdf_entry>::value)
        hipLaunchKernelGGL(tsdf_compact_kernel, grid, dim3(256), 0, s, t->t, min_weight, out, (unsigned long long)out_cap);
    else
        hipLaunchKernelGGL(tsdf_crossings_kernel, grid, dim3(256), 0, s, t->t, min_weight, out, (unsigned long long)out_cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(n, t->t.words + TSDF_W_OUT, sizeof(*n), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VISO_OK;
}

static inline unsigned long long host_key(const int32_t* k) {
    return ((unsigned long long)(uint32_t)(k[0] + MAP_BIAS) << 42) | ((unsigned long long)(uint32_t)(k[1] + MAP_BIAS) << 21) |
           (unsigned long long)(uint32_t)(k[2] + MAP_BIAS);
}
static inline bool item_less(const viso_tsdf_entry& x, const viso_tsdf_entry& y) { return host_key(x.k) < host_key(y.k); }
static inline bool item_less(const viso_tsdf_crossing& x, const viso_tsdf_crossing& y) {
    const unsigned long long a = host_key(x.k), b = host_key(y.k);
    return a != b ? a < b : x.axis < y.axis;
}

// the count (out_items == null and n_cap == 0 with count_only) or the sorted list of an extraction
template <class Item>
static int tsdf_extract(const char* where, viso_tsdf* t, uint32_t min_weight, bool count_only, Item* items_out, size_t n_cap, size_t* n) {
    if (!tsdf_known(t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    if (!n || min_weight < 1 || (!count_only && n_cap && !items_out)) { viso_set_error("%s: bad argument (min_weight >= 1, non-null outputs)", where); return VISO_ERR_ARG; }
    int r;
    if ((r = tsdf_enter(where, t)) < 0) return r;
    std::lock_guard<std::mutex> lk(t->mu);
    if (t->overflowed) return tsdf_refuse_overflowed(where);
    unsigned long long c = 0;
    if ((r = tsdf_pass<Item>(t, min_weight, nullptr, 0, &c)) < 0) return r;
    *n = (size_t)c;
    if (count_only || !c) return VISO_OK;
    if (c > n_cap) { viso_set_error("%s: %llu items do not fit the %zu given", where, c, n_cap); return VISO_ERR_ARG; }
    Item* d = nullptr;
    if (hipMalloc((void**)&d, (size_t)c * sizeof(Item)) != hipSuccess) {
        (void)hipGetLastError();
        viso_set_error("%s: cannot allocate %zu bytes for the list", where, (size_t)c * sizeof(Item));
        return VISO_ERR_NOMEM;
    }
    unsigned long long c2 = 0;
    r = tsdf_pass<Item>(t, min_weight, d, (size_t)c, &c2);
    hipError_t e = hipSuccess;
    if (r >= 0) e = hipMemcpy(items_out, d, (size_t)c * sizeof(Item), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (r < 0) return r;
    HIP_TRY(e);
    if (c2 != c) { viso_set_error("%s: the table changed between the two passes", where); return VISO_ERR_HIP; }   // (the map's lock rules it out)
    std::sort(items_out, items_out + c, [](const Item& x, const Item& y) { return item_less(x, y); });
    return VISO_OK;
}

extern "C" int viso_tsdf_count(viso_tsdf* t, uint32_t min_weight, size_t* n) {
    return tsdf_extract<viso_tsdf_entry>("viso_tsdf_count", t, min_weight, true, nullptr, 0, n);
}
extern "C" int viso_tsdf_get(viso_tsdf* t, uint32_t min_weight, viso_tsdf_entry* entries_out, size_t n_cap, size_t* n) {
    return tsdf_extract<viso_tsdf_entry>("viso_tsdf_get", t, min_weight, false, entries_out, n_cap, n);
}
extern "C" int viso_tsdf_surface_count(viso_tsdf* t, uint32_t min_weight, size_t* n) {
    return tsdf_extract<viso_tsdf_crossing>("viso_tsdf_surface_count", t, min_weight, true, nullptr, 0, n);
}
extern "C" int viso_tsdf_surface(viso_tsdf* t, uint32_t min_weight, viso_tsdf_crossing* crossings_out, size_t n_cap, size_t* n) {
    return tsdf_extract<viso_tsdf_crossing>("viso_tsdf_surface", t, min_weight, false, crossings_out, n_cap, n);
}

// One pass of the mesh extraction: the numbers of vertex records and of triangles, both lists written when `verts` is set
static int tsdf_mesh_pass(viso_tsdf* t, uint32_t min_weight, viso_tsdf_mesh_vertex* verts, size_t v_cap, TsdfTriRef* tris, size_t t_cap,
                          unsigned long long* nv, unsigned long long* nt) {
    hipStream_t s = t->ctx->stream;
    HIP_TRY(hipMemsetAsync(t->t.words + TSDF_W_OUT, 0, sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(t->t.words + TSDF_W_TRIS, 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(tsdf_mesh_kernel, dim3((t->t.mask + 1u) / 256u), dim3(256), 0, s, t->t, min_weight, t->s, verts,
                       (unsigned long long)v_cap, tris, (unsigned long long)t_cap);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(nv, t->t.words + TSDF_W_OUT, sizeof(*nv), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(nt, t->t.words + TSDF_W_TRIS, sizeof(*nt), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VISO_OK;
}

static inline bool vertex_less(const viso_tsdf_mesh_vertex& x, const viso_tsdf_mesh_vertex& y) {
    const unsigned long long a = host_key(x.k), b = host_key(y.k);
    return a != b ? a < b : x.dir < y.dir;
}

// The map is entered and locked.  Both lists from the device, sorted; the vertices no triangle refers to dropped; the references
// turned into indices.
static int tsdf_mesh_lists(const char* where, viso_tsdf* t, uint32_t min_weight, std::vector<viso_tsdf_mesh_vertex>& verts,
                           std::vector<viso_tsdf_triangle>& tris) {
    verts.clear(); tris.clear();
    unsigned long long nv = 0, nt = 0;
    int r;
    if ((r = tsdf_mesh_pass(t, min_weight, nullptr, 0, nullptr, 0, &nv, &nt)) < 0) return r;
    if (!nt) return VISO_OK;   // no triangle: no vertex is referred to
    std::vector<viso_tsdf_mesh_vertex> all((size_t)nv);
    std::vector<TsdfTriRef> refs((size_t)nt);
    viso_tsdf_mesh_vertex* dv = nullptr;
    TsdfTriRef* dt = nullptr;
    const size_t bv = (size_t)nv * sizeof(viso_tsdf_mesh_vertex), bt = (size_t)nt * sizeof(TsdfTriRef);
    if (hipMalloc((void**)&dv, bv) != hipSuccess || hipMalloc((void**)&dt, bt) != hipSuccess) {
        (void)hipGetLastError();
        if (dv) (void)hipFree(dv);
        viso_set_error("%s: cannot allocate %zu bytes for the lists", where, bv + bt);
        return VISO_ERR_NOMEM;
    }
    unsigned long long nv2 = 0, nt2 = 0;
    r = tsdf_mesh_pass(t, min_weight, dv, (size_t)nv, dt, (size_t)nt, &nv2, &nt2);
    hipError_t e = hipSuccess;
    if (r >= 0) e = hipMemcpy(all.data(), dv, bv, hipMemcpyDeviceToHost);
    if (r >= 0 && e == hipSuccess) e = hipMemcpy(refs.data(), dt, bt, hipMemcpyDeviceToHost);
    (void)hipFree(dv);
    (void)hipFree(dt);
    if (r < 0) return r;
    HIP_TRY(e);
    if (nv2 != nv || nt2 != nt) { viso_set_error("%s: the table changed between the two passes", where); return VISO_ERR_HIP; }   // (the map's lock rules it out)
    std::sort(all.begin(), all.end(), vertex_less);
    std::sort(refs.begin(), refs.end(), [](const TsdfTriRef& x, const TsdfTriRef& y) { return x.cell != y.cell ? x.cell < y.cell : (x.code & 15u) < (y.code & 15u); });
    // every reference to the position of its vertex in the sorted list
    std::vector<unsigned long long> at((size_t)nt * 3);
    std::vector<unsigned char> used((size_t)nv, 0);
    for (size_t i = 0; i < (size_t)nt; ++i) {
        for (int m = 0; m < 3; ++m) {
            const uint32_t v = (refs[i].code >> (4 + 6 * m)) & 63u, c = v >> 3;
            const unsigned long long key = refs[i].cell + ((unsigned long long)(c & 1u) << 42) + ((unsigned long long)((c >> 1) & 1u) << 21) + (unsigned long long)(c >> 2);
            const int dir = (int)(v & 7u);
            size_t lo = 0, hi = (size_t)nv;
            while (lo < hi) {
                const size_t mid = lo + (hi - lo) / 2;
                const unsigned long long km = host_key(all[mid].k);
                if (km < key || (km == key && all[mid].dir < dir)) lo = mid + 1; else hi = mid;
            }
            if (lo == (size_t)nv || host_key(all[lo].k) != key || all[lo].dir != dir) {
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

static int tsdf_mesh_extract(const char* where, viso_tsdf* t, uint32_t min_weight, bool count_only, viso_tsdf_mesh_vertex* vertices_out,
                             size_t nv_cap, viso_tsdf_triangle* triangles_out, size_t nt_cap, size_t* n_vertices, size_t* n_triangles) {
    if (!tsdf_known(t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    if (!n_vertices || !n_triangles || min_weight < 1 || (!count_only && ((nv_cap && !vertices_out) || (nt_cap && !triangles_out)))) {
        viso_set_error("%s: bad argument (min_weight >= 1, non-null outputs)", where);
        return VISO_ERR_ARG;
    }
    int r;
    if ((r = tsdf_enter(where, t)) < 0) return r;
    std::vector<viso_tsdf_mesh_vertex> verts;
    std::vector<viso_tsdf_triangle> tris;
    {
        std::lock_guard<std::mutex> lk(t->mu);
        if (t->overflowed) return tsdf_refuse_overflowed(where);
        if ((r = tsdf_mesh_lists(where, t, min_weight, verts, tris)) < 0) return r;
    }
    *n_vertices = verts.size();
    *n_triangles = tris.size();
    if (count_only) return VISO_OK;
    if (verts.size() > nv_cap || tris.size() > nt_cap) {
        viso_set_error("%s: %zu vertices and %zu triangles do not fit the %zu and %zu given", where, verts.size(), tris.size(), nv_cap, nt_cap);
        return VISO_ERR_ARG;
    }
    std::copy(verts.begin(), verts.end(), vertices_out);
    std::copy(tris.begin(), tris.end(), triangles_out);
    return VISO_OK;
}

extern "C" int viso_tsdf_mesh_count(viso_tsdf* t, uint32_t min_weight, size_t* n_vertices, size_t* n_triangles) {
    return tsdf_mesh_extract("viso_tsdf_mesh_count", t, min_weight, true, nullptr, 0, nullptr, 0, n_vertices, n_triangles);
}
extern "C" int viso_tsdf_mesh(viso_tsdf* t, uint32_t min_weight, viso_tsdf_mesh_vertex* vertices_out, size_t nv_cap,
                              viso_tsdf_triangle* triangles_out, size_t nt_cap, size_t* n_vertices, size_t* n_triangles) {
    return tsdf_mesh_extract("viso_tsdf_mesh", t, min_weight, false, vertices_out, nv_cap, triangles_out, nt_cap, n_vertices, n_triangles);
}

extern "C" int viso_tsdf_stats(viso_tsdf* t, viso_tsdf_counters* out) {
    const char* where = "viso_tsdf_stats";
    if (!tsdf_known(t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    if (!out) { viso_set_error("%s: bad argument (a non-null output)", where); return VISO_ERR_ARG; }
    int r;
    if ((r = tsdf_enter(where, t)) < 0) return r;
    std::lock_guard<std::mutex> lk(t->mu);
    std::vector<unsigned long long> h((size_t)TSDF_STAT_SETS * TSDF_STAT_WORDS + 2);
    hipStream_t s = t->ctx->stream;
    HIP_TRY(hipMemcpyAsync(h.data(), t->t.stats, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));   // stats | words: adjacent
    HIP_TRY(hipStreamSynchronize(s));
    viso_tsdf_counters c = {0, 0, 0, 0, 0};
    for (int k = 0; k < TSDF_STAT_SETS; ++k) {
        const unsigned long long* st = h.data() + (size_t)k * TSDF_STAT_WORDS;
        c.n_points += st[TSDF_ST_POINTS]; c.n_updates += st[TSDF_ST_UPDATES]; c.n_out_of_range += st[TSDF_ST_OOR]; c.n_occupied += st[TSDF_ST_OCC];
    }
    c.n_dropped = h[(size_t)TSDF_STAT_SETS * TSDF_STAT_WORDS + TSDF_W_DROPPED];
    *out = c;
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
