// voxel_hash.h — the key, the hash and the probes of the hash tables of voxels (voxelmap.hip, tsdf.hip; include/viso_hip.h,
// "voxel map" step 4 and "Full table").  Device only.  A table's keys are [mask + 1] u64, all ones = empty; a key is claimed with
// one 64-bit compare-and-swap.  Every probe loop visits each slot at most once and advances strictly: a full table is a wrong count,
// never a hang.
#ifndef VISO_VOXEL_HASH_H_
#define VISO_VOXEL_HASH_H_
#include "common.h"

#define MAP_EMPTY 0xffffffffffffffffull
#define MAP_BIAS (1 << 20)
#define MAP_RANGE 1073741824.0          // 2^30: |g| at and beyond it is out of range

__device__ __forceinline__ uint32_t map_hash(unsigned long long k) {   // the finaliser of splitmix64
    k ^= k >> 30; k *= 0xbf58476d1ce4e5b9ull;
    k ^= k >> 27; k *= 0x94d049bb133111ebull;
    k ^= k >> 31;
    return (uint32_t)k;
}

__device__ __forceinline__ unsigned long long map_key(int kx, int ky, int kz) {
    return ((unsigned long long)(uint32_t)(kx + MAP_BIAS) << 42) | ((unsigned long long)(uint32_t)(ky + MAP_BIAS) << 21) |
           (unsigned long long)(uint32_t)(kz + MAP_BIAS);
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
#endif /* VISO_VOXEL_HASH_H_ */
