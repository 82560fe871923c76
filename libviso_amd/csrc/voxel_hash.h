// voxel_hash.h — the device side of the shared table layer of the hash tables of voxels (voxelmap.hip, tsdf.hip; the host side is
// voxel_host.h; include/viso_hip.h, "voxel map" step 4 and "Full table").  A table's keys are [mask + 1] u64, all
// ones = empty; a key is claimed with one 64-bit compare-and-swap.  Every probe loop visits each slot at most once and advances
// strictly: a full table is a wrong count, never a hang.  Beside the keys every table has 256 sets of counters on cache lines of
// their own (a workgroup adds to set blockIdx & 255, one atomic per wave and counter; summed on the host) and a few single words.
// What is in a slot is the kind's payload P (below); the kernels that only list, zero or add to slots are here once for every kind,
// templates over P: voxel_compact_kernel, voxel_clear_kernel, voxel_add_entries_kernel and the three of an eviction
// (include/viso_hip.h, "Map eviction"), and the check and the mark of a retract ("TSDF retract"), whose
// tombstones the eviction's rebuild and sweep take away.  Only the two marks and the rebuild ever write a tombstone, and none is left
// when a call is done.
#ifndef VISO_VOXEL_HASH_H_
#define VISO_VOXEL_HASH_H_
#include "common.h"

#define MAP_EMPTY 0xffffffffffffffffull
#define MAP_TOMB 0xfffffffffffffffeull   // an evicted slot between the passes of an eviction (keys are 63 bits); never outlives the call
#define MAP_BIAS (1 << 20)
#define MAP_RANGE 1073741824.0          // 2^30: |g| at and beyond it is out of range

#define VOXEL_STAT_SETS 256
#define VOXEL_STAT_WORDS 16             // 128 bytes a set
#define VOXEL_ST_POINTS 0
#define VOXEL_ST_UPDATES 1              // the voxel map's inserts, the TSDF map's updates
#define VOXEL_ST_OOR 2
#define VOXEL_ST_OCC 3
#define VOXEL_ST_FREED 4                // the slots that the checks of the retracts since the last clear found freed / bad: running counts,
#define VOXEL_ST_BAD 5                  // of which a call takes the difference; no getter reads them, and they are no part of the map
#define VOXEL_W_OUT 0                   // words: an extraction's list length
#define VOXEL_W_DROPPED 1               //        points / updates that found no slot
#define VOXEL_W_TRIS 2                  //        the mesh's triangle list length (VOXEL_W_OUT: its vertex list's)
#define VOXEL_W_MISSING 3               //        a retract's updates whose voxel is not in the table
#define VOXEL_W_UNDERFLOW 4             //        not zero: a retract took a voxel's weight below zero (how many atomics saw it: scheduling)
#define VOXEL_WORDS 5                   // how many of them there are; the table's allocation has room for 32 (voxel_create)
#define VOXEL_MAX_PIXELS 0x7fffffffll
#define VOXEL_GROUP 16384               // frames along a grid's y

// the head of every table; a table embeds it as its first member, next to its payload arrays
struct VoxelTable {
    unsigned long long* keys;
    unsigned long long* stats;   // [VOXEL_STAT_SETS][VOXEL_STAT_WORDS]
    unsigned long long* words;   // VOXEL_W_*, behind the stats
    uint32_t mask;               // slots - 1
};

// what every fuse kernel takes: the maps, the poses and the calibration
struct VoxelFuseArgs {
    const int16_t* disp; size_t mfs;   // frame f's map at disp + f * mfs
    const double* poses;               // [frames][12] on the device, or null: no transform
    int rows, cols, min_disp16, _pad;
    double f, cu, cv, base;
};

__host__ __device__ __forceinline__ unsigned long long voxel_key(int kx, int ky, int kz) {
    return ((unsigned long long)(uint32_t)(kx + MAP_BIAS) << 42) | ((unsigned long long)(uint32_t)(ky + MAP_BIAS) << 21) |
           (unsigned long long)(uint32_t)(kz + MAP_BIAS);
}
__host__ __device__ __forceinline__ void voxel_unkey(unsigned long long key, int32_t* k) {
    for (int i = 0; i < 3; ++i) k[i] = (int)((key >> (21 * (2 - i))) & 0x1fffffu) - MAP_BIAS;
}
// the key of the voxel at the corner d = dx + 2 dy + 4 dz of key's cell (no field of key is at its last value along a set bit of d)
__host__ __device__ __forceinline__ unsigned long long voxel_neighbour(unsigned long long key, uint32_t d) {
    return key + voxel_key((int)(d & 1u) - MAP_BIAS, (int)((d >> 1) & 1u) - MAP_BIAS, (int)(d >> 2) - MAP_BIAS);
}
// the key one voxel up / down along axis ax (0: x, 1: y, 2: z); false: key is at the last / the first index of that axis, which has
// no neighbour there (the upper end is the rule of tsdf_crossings_kernel, the lower end its twin)
__host__ __device__ __forceinline__ bool voxel_step_up(unsigned long long key, int ax, unsigned long long* out) {
    const int sh = 21 * (2 - ax);
    if (((key >> sh) & 0x1fffffull) == 0x1fffffull) return false;
    *out = key + (1ull << sh);
    return true;
}
__host__ __device__ __forceinline__ bool voxel_step_down(unsigned long long key, int ax, unsigned long long* out) {
    const int sh = 21 * (2 - ax);
    if (((key >> sh) & 0x1fffffull) == 0ull) return false;
    *out = key - (1ull << sh);
    return true;
}

__device__ __forceinline__ uint32_t map_hash(unsigned long long k) {   // the finaliser of splitmix64
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return (uint32_t)k;
}

// The slot of `key`, claimed if the key is new.  false: every slot holds another key.
__device__ __forceinline__ bool voxel_probe(unsigned long long* keys, uint32_t mask, unsigned long long key, uint32_t* slot_out, bool* claimed) {
    uint32_t slot = map_hash(key) & mask;
    for (uint32_t n = 0; n <= mask; ++n, slot = (slot + 1) & mask) {   // at most one visit of every slot
        unsigned long long cur = __hip_atomic_load(keys + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == MAP_EMPTY) {
            cur = atomicCAS(keys + slot, MAP_EMPTY, key);
            if (cur == MAP_EMPTY) { *claimed = true; *slot_out = slot; return true; }
        }
        if (cur == key) { *slot_out = slot; return true; }
    }
    return false;
}

// The slot of `key` in a table that nothing writes meanwhile; false: the key is not in it.  Reads only.
__device__ __forceinline__ bool voxel_find(const unsigned long long* keys, uint32_t mask, unsigned long long key, uint32_t* slot_out) {
    uint32_t slot = map_hash(key) & mask;
    for (uint32_t n = 0; n <= mask; ++n, slot = (slot + 1) & mask) {   // at most one visit of every slot
        const unsigned long long cur = keys[slot];
        if (cur == key) { *slot_out = slot; return true; }
        if (cur == MAP_EMPTY) return false;
    }
    return false;
}

// Pixel i of frame `frame` to its point in the camera's coordinates.  false (X, Y, Z untouched): beyond the map, invalid or below
// min_disp16.
__device__ __forceinline__ bool voxel_point(const VoxelFuseArgs& a, size_t i, int frame, double* X, double* Y, double* Z) {
    if (i >= (size_t)a.rows * a.cols) return false;
    const int d16 = a.disp[(size_t)frame * a.mfs + i];
    if (d16 == VISO_DISP_INVALID || d16 < a.min_disp16) return false;
    const int y = (int)(i / (size_t)a.cols), x = (int)(i - (size_t)y * a.cols);
    const double d = (double)d16 / 16.0;
    *X = a.base * ((double)x - a.cu) / d;      // the operand order of points_kernel (speckle.hip)
    *Y = a.base * ((double)y - a.cv) / d;
    *Z = a.f * a.base / d;
    return true;
}

// The runs of equal keys along the wave: `head` in the first lane of a run, `len` the number of lanes from this one to the end of
// its run (in a head lane: the run's length).  Every lane of the wave calls.
__device__ __forceinline__ void voxel_runs(unsigned long long key, int lane, bool* head, uint32_t* len) {
    const unsigned long long kl = __shfl_up(key, 1);
    *head = lane == 0 || key != kl;
    const unsigned long long m = __ballot(*head);
    const unsigned long long above = lane < 63 ? m >> (lane + 1) : 0ull;
    *len = above ? (uint32_t)__ffsll((long long)above) : (uint32_t)(64 - lane);
}

// The first lane of this lane's run, from the `head` of voxel_runs: the highest head lane at or below this one (lane 0 is a head).
// Every lane of the wave calls.
__device__ __forceinline__ int voxel_run_head(bool head, int lane) {
    const unsigned long long m = __ballot(head) & (~0ull >> (63 - lane));
    return 63 - __clzll((long long)m);
}

__device__ __forceinline__ unsigned long long* voxel_stat(const VoxelTable& t, unsigned block, int which) {
    return t.stats + (size_t)(block & (VOXEL_STAT_SETS - 1)) * VOXEL_STAT_WORDS + which;
}

// A wave's totals into the block's set: one atomic per counter that is not zero, from lane 0.
__device__ __forceinline__ void voxel_count_wave(const VoxelTable& t, unsigned block, int lane, unsigned long long points,
                                                 unsigned long long updates, unsigned long long oor, unsigned long long occ) {
    if (lane == 0) {
        if (points) atomicAdd(voxel_stat(t, block, VOXEL_ST_POINTS), points);
        if (updates) atomicAdd(voxel_stat(t, block, VOXEL_ST_UPDATES), updates);
        if (oor) atomicAdd(voxel_stat(t, block, VOXEL_ST_OOR), oor);
        if (occ) atomicAdd(voxel_stat(t, block, VOXEL_ST_OCC), occ);
    }
}

// The position in the list of VOXEL_W_OUT of a lane that takes one: one atomic per wave.  false: no lane of the wave takes one.
// Every lane of the wave calls.
__device__ __forceinline__ bool voxel_list_position(const VoxelTable& t, bool take, int lane, unsigned long long* at) {
    const unsigned long long m = __ballot(take);
    if (!m) return false;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(t.words + VOXEL_W_OUT, (unsigned long long)__popcll(m));
    base = __shfl(base, 0);
    *at = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
    return true;
}

// ---- a kind's payload ------------------------------------------------------------------------------------------------------------
// P is a small struct by value, the only place that knows the kind's arrays and the layout of its entries:
//   typename P::Entry            a slot as the kind's getters list it
//   head()                       the table's VoxelTable
//   threshold(slot)              the word the getters compare with min_count / min_weight
//   pack(slot, key, w, Entry*)   the slot as an entry; w: its threshold word, which the caller has read
//   zero(a), move(a, b)          slot a's payload words zeroed; moved to slot b, slot a's zeroed
//   key(entry), add(slot, entry) an entry's key; the entry's atomic adds to the slot a probe gave it
//   units(entry)                 what the entry stands for (its count / weight): added to VOXEL_W_DROPPED when it finds no slot,
//                                else to the counter P::UNITS_STAT; with P::ENTRY_STAT every entry also counts one in VOXEL_ST_UPDATES
// and, only of a kind that can be retracted from (the TSDF map's two; the voxel map has neither):
//   is_zero(slot)                every payload word of the slot but its threshold word is 0
//   within(slot, w, bound)       the slot, of threshold word w >= 1, is one that valid entries of the kind add up to

// One thread per slot (the grid covers the slots exactly: at least 1024 of them): the occupied slots whose threshold word is at
// least `min` to a dense list, one atomic per wave for the positions.  out == null: only their number.
template <class P>
__global__ __launch_bounds__(256) void voxel_compact_kernel(P p, uint32_t min, typename P::Entry* out, unsigned long long out_cap) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long key = p.head().keys[slot];
    const uint32_t w = p.threshold(slot);
    const bool take = key != MAP_EMPTY && w >= min;
    unsigned long long at;
    if (!voxel_list_position(p.head(), take, threadIdx.x & 63, &at)) return;   // the whole wave
    if (take && out && at < out_cap) {
        typename P::Entry v;
        p.pack(slot, key, w, &v);
        out[at] = v;
    }
}

// One thread per slot: the key to empty, the payload, the counters and the words to zero.
template <class P>
__global__ __launch_bounds__(256) void voxel_clear_kernel(P p) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    const VoxelTable& t = p.head();
    t.keys[slot] = MAP_EMPTY;
    for (uint32_t w = slot; w < VOXEL_STAT_SETS * VOXEL_STAT_WORDS; w += t.mask + 1u) t.stats[w] = 0ull;   // (the smallest table has fewer slots)
    if (slot < VOXEL_WORDS) t.words[slot] = 0ull;
    p.zero(slot);
}

// An entry into the slot of its key, claimed if the key is new; an entry that finds no slot counts as dropped.
template <class P>
__device__ __forceinline__ void voxel_insert(const P& p, const typename P::Entry& v, bool* claimed) {
    uint32_t slot;
    if (voxel_probe(p.head().keys, p.head().mask, P::key(v), &slot, claimed)) p.add(slot, v);
    else atomicAdd(p.head().words + VOXEL_W_DROPPED, P::units(v));
}

// One thread per entry, through the probe of the fuse kernels.
template <class P>
__global__ __launch_bounds__(256) void voxel_add_entries_kernel(P p, const typename P::Entry* e, unsigned long long n) {
    const unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const VoxelTable& t = p.head();
    const bool on = i < n;
    bool claimed = false;
    if (on) {
        const typename P::Entry v = e[i];
        const unsigned long long u = P::units(v);
        voxel_insert(p, v, &claimed);
        atomicAdd(voxel_stat(t, blockIdx.x, P::UNITS_STAT), u);
    }
    voxel_count_wave(t, blockIdx.x, threadIdx.x & 63, 0, P::ENTRY_STAT ? __popcll(__ballot(on)) : 0, 0, __popcll(__ballot(claimed)));
}

// ---- eviction: the voxels outside a box leave the table, in place ----------------------------------------------------------------
struct VoxelBox { int32_t lo[3], hi[3]; };   // viso_voxel_box: voxel k is inside when lo[i] <= k[i] < hi[i]

__device__ __forceinline__ bool voxel_in_box(unsigned long long key, const VoxelBox& b) {
    int32_t k[3];
    voxel_unkey(key, k);
    return k[0] >= b.lo[0] && k[0] < b.hi[0] && k[1] >= b.lo[1] && k[1] < b.hi[1] && k[2] >= b.lo[2] && k[2] < b.hi[2];
}

#define VOXEL_EVICT_COUNT 0   // the number of voxels outside the box; reads only
#define VOXEL_EVICT_LIST 1    // those voxels to `out` (null: nowhere), their keys to MAP_TOMB
#define VOXEL_EVICT_KEEP 2    // the voxels inside the box to `out`; reads only (the full table's way out)
#define VOXEL_EVICT_PEEK 3    // the voxels outside the box to `out`; reads only (the same)

// Pass 1, one thread per slot (the grid covers the slots exactly).  Positions come from voxel_list_position, one atomic per wave.
template <class P>
__global__ __launch_bounds__(256) void voxel_evict_mark_kernel(VoxelTable t, P p, VoxelBox box, int mode, typename P::Entry* out,
                                                               unsigned long long out_cap) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    const unsigned long long key = t.keys[slot];
    const bool live = key < MAP_TOMB;
    const bool take = live && voxel_in_box(key, box) == (mode == VOXEL_EVICT_KEEP);
    unsigned long long at;
    if (!voxel_list_position(t, take, threadIdx.x & 63, &at)) return;   // the whole wave
    if (!take || mode == VOXEL_EVICT_COUNT) return;
    if (out) {
        if (at >= out_cap) return;   // (a list of the first pass's length has room for all: the slot stays as it is)
        typename P::Entry v;
        p.pack(slot, key, p.threshold(slot), &v);
        out[at] = v;
    }
    if (mode == VOXEL_EVICT_LIST) t.keys[slot] = MAP_TOMB;
}

// Pass 2, one thread per slot; only the thread of a cluster's first slot (its own not empty, the one before it, cyclically, empty)
// goes on, and walks its cluster in slot order to the next empty slot.  Every live entry is put back at the first tombstone at or
// after its home slot, which is never later than the slot it is in; the slot it leaves becomes a tombstone.  So behind the walk no
// tombstone lies between an entry's home and its slot, and the sweep may empty them all.  The pass writes MAP_EMPTY nowhere and
// reads nothing beyond its own cluster (a home before the cluster's head, which only a bad table has, counts as the head), so the
// walkers are independent and which slots are heads does not change while they run.  Offsets count from the head; `ft`: no
// tombstone lies at an offset below it.  Both loops advance strictly: the outer one visits every slot of the cluster once, the
// inner one the slots from the entry's home (or ft) to its own.  A table without an empty slot has no head: the host does not come
// here with one.
template <class P>
__global__ __launch_bounds__(256) void voxel_evict_rebuild_kernel(VoxelTable t, P p) {
    const uint32_t head = blockIdx.x * 256 + threadIdx.x, mask = t.mask;
    unsigned long long* keys = t.keys;
    if (keys[head] == MAP_EMPTY || keys[(head - 1u) & mask] != MAP_EMPTY) return;
    uint32_t ft = 0;
    for (uint32_t n = 0; n <= mask; ++n) {
        const uint32_t s = (head + n) & mask;
        const unsigned long long k = keys[s];
        if (k == MAP_EMPTY) break;
        if (k == MAP_TOMB) continue;
        const uint32_t d = (s - (map_hash(k) & mask)) & mask;   // slots from its home to here
        uint32_t o = d <= n ? n - d : 0u;
        const bool from_ft = o <= ft;
        if (from_ft) o = ft;
        while (o < n && keys[(head + o) & mask] != MAP_TOMB) ++o;
        if (o < n) {
            const uint32_t to = (head + o) & mask;
            keys[to] = k;
            p.move(s, to);
            keys[s] = MAP_TOMB;
        }
        if (from_ft) ft = o + 1u;
    }
}

// Pass 3, one thread per slot: every tombstone to MAP_EMPTY, its payload zeroed as voxel_clear_kernel does.
template <class P>
__global__ __launch_bounds__(256) void voxel_evict_sweep_kernel(VoxelTable t, P p) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (t.keys[slot] != MAP_TOMB) return;
    p.zero(slot);
    t.keys[slot] = MAP_EMPTY;
}

// ---- retract: the slots whose payload a take brought back to zero leave the table (include/viso_hip.h, "TSDF retract") -----------
#define VOXEL_SLOT_KEEP 0    // empty, or live and within the kind's bounds
#define VOXEL_SLOT_FREED 1   // live, its threshold word 0 and every other payload word 0: what is left of a voxel all of whose updates were taken
#define VOXEL_SLOT_BAD 2     // live and not a slot that entries of the kind add up to: the threshold word 0 beside another word that is not,
                             // or a payload beyond the kind's bounds

// what a retract's check makes of a slot; bound: what P::within compares with
template <class P>
__device__ __forceinline__ int voxel_slot_state(const VoxelTable& t, const P& p, uint32_t slot, long long bound) {
    if (t.keys[slot] >= MAP_TOMB) return VOXEL_SLOT_KEEP;
    const uint32_t w = p.threshold(slot);
    if (!w) return p.is_zero(slot) ? VOXEL_SLOT_FREED : VOXEL_SLOT_BAD;
    return p.within(slot, w, bound) ? VOXEL_SLOT_KEEP : VOXEL_SLOT_BAD;
}

// The check, one thread per slot (the grid covers the slots exactly), reads the table only: the freed and the bad slots counted in
// VOXEL_ST_FREED and VOXEL_ST_BAD of the block's set, one atomic per wave and counter that is not zero.  (Not in one word, as the
// extractions count: a retract of many frames frees a slot in most waves, and their atomics on one address would be the call.)
template <class P>
__global__ __launch_bounds__(256) void voxel_retract_check_kernel(VoxelTable t, P p, long long bound) {
    const int state = voxel_slot_state(t, p, blockIdx.x * 256 + threadIdx.x, bound);
    const unsigned long long freed = __ballot(state == VOXEL_SLOT_FREED), bad = __ballot(state == VOXEL_SLOT_BAD);
    if ((threadIdx.x & 63) != 0) return;
    if (freed) atomicAdd(voxel_stat(t, blockIdx.x, VOXEL_ST_FREED), (unsigned long long)__popcll(freed));
    if (bad) atomicAdd(voxel_stat(t, blockIdx.x, VOXEL_ST_BAD), (unsigned long long)__popcll(bad));
}

// The mark, one thread per slot, behind a check that found no bad slot: the key of every freed slot to MAP_TOMB.
// voxel_evict_rebuild_kernel and voxel_evict_sweep_kernel follow before anything else can return.
template <class P>
__global__ __launch_bounds__(256) void voxel_retract_mark_kernel(VoxelTable t, P p, long long bound) {
    const uint32_t slot = blockIdx.x * 256 + threadIdx.x;
    if (voxel_slot_state(t, p, slot, bound) == VOXEL_SLOT_FREED) t.keys[slot] = MAP_TOMB;
}
#endif /* VISO_VOXEL_HASH_H_ */
