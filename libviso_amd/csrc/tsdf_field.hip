// tsdf_field.hip — the exact distance field of a TSDF map's surface over a box of voxels (include/viso_hip.h, "TSDF distance
// field"): for every cell of the box the squared distance, in voxels and as an integer, to the nearest site of the
// box.  Opt-in, NOT in the reference.  The definition is the header's; the device output is bit-identical to tests/field_ref.py.
//
// Four launches over the cells of the box, one thread per cell, the cells of a wave adjacent along axis 2 (cell (i0, i1, i2) is at
// (i0 n1 + i1) n2 + i2, so consecutive lanes are consecutive words):
//   tsdf_field_sites_kernel   the cell's own read-only probe and at most six for its neighbours: the state, the starting value
//                             (0 at a site, VISO_FIELD_NONE elsewhere) and the number of sites, one ballot a round and one atomic
//                             per wave.  At most 2048 blocks, each taking 256 cells a round: with one wave per 64 cells, a box
//                             whose unknown cells are sites sent 262144 atomics to one word, 2.8 of the kernel's 3.2 ms
//   tsdf_field_pass_kernel    three times, along axis 2, 1 and 0: g'(i) = min_j g(j) + (i - j)^2 along the cell's line, from one
//                             buffer into the other (a line is read whole from the buffer that no thread of the launch writes).  The
//                             minimum is searched outward from i, both sides at once, and the search ends once d^2 >= the best
//                             value so far: nothing further out can be smaller.  The lanes of a wave sit on neighbouring lines (or
//                             on neighbouring cells of one line), so every step is one coalesced load a side.
// The three one-dimensional minima composed are the minimum over the box of the sum of the three squares: the exact Euclidean
// transform.  VISO_FIELD_NONE is never added to; a finite value stays below 3 * 511^2 < 2^20.
// Every loop is bounded by an axis length (<= 512), by the 256 rounds of the sites kernel, or is the probe's one round of the
// slots.  Device memory of a call: two uint32 and one uint8 a cell.  No LDS, no scratch.
#include "common.h"
#include "tsdf_field.h"

#define FIELD_SITE_BLOCKS 2048   // the grid of the sites kernel: with the 2^27 cells of the largest box, 256 rounds a block
#define FIELD_STATE_FRONT 1u
#define FIELD_STATE_BEHIND 2u

// weight >= min_weight of the voxel `key` in the table: *neg = (sum < 0).  One read-only probe.
__device__ __forceinline__ bool field_usable(const TsdfTable& t, unsigned long long key, uint32_t min_weight, bool* neg) {
    uint32_t slot;
    if (!voxel_find(t.head.keys, t.head.mask, key, &slot)) return false;
    if (t.weight[slot] < min_weight) return false;
    *neg = (long long)t.sum[slot] < 0;
    return true;
}

// a usable neighbour one step along AX (UP: upwards) of the other sign; the first and the last index of an axis have no neighbour
// on that side
template <int AX, bool UP>
__device__ __forceinline__ bool field_crosses(const TsdfTable& t, unsigned long long key, uint32_t min_weight, bool neg) {
    unsigned long long kn;
    if (!(UP ? voxel_step_up(key, AX, &kn) : voxel_step_down(key, AX, &kn))) return false;
    bool nn;
    return field_usable(t, kn, min_weight, &nn) && nn != neg;
}

__global__ __launch_bounds__(256) void tsdf_field_sites_kernel(TsdfTable t, uint32_t min_weight, FieldBox b, uint32_t unknown_is_site,
                                                               uint32_t* g, uint8_t* state) {
    uint32_t sites = 0;   // of this wave, the same in all its lanes
    // a block takes 256 cells at a time, the grid's blocks apart: at most 256 times (the host sizes the grid: FIELD_SITE_BLOCKS)
    for (uint32_t base = blockIdx.x * 256; base < b.cells; base += gridDim.x * 256) {
        const uint32_t c = base + threadIdx.x;
        bool site = false;
        if (c < b.cells) {
            const uint32_t i2 = c % b.n[2], r = c / b.n[2], i1 = r % b.n[1], i0 = r / b.n[1];
            const long long k0 = (long long)b.lo[0] + i0, k1 = (long long)b.lo[1] + i1, k2 = (long long)b.lo[2] + i2;
            uint32_t st = 0;
            if (k0 >= -MAP_BIAS && k0 < MAP_BIAS && k1 >= -MAP_BIAS && k1 < MAP_BIAS && k2 >= -MAP_BIAS && k2 < MAP_BIAS) {
                const unsigned long long key = voxel_key((int)k0, (int)k1, (int)k2);
                bool neg;
                if (field_usable(t, key, min_weight, &neg)) {
                    st = neg ? FIELD_STATE_BEHIND : FIELD_STATE_FRONT;
                    if (field_crosses<0, true>(t, key, min_weight, neg) || field_crosses<0, false>(t, key, min_weight, neg) ||
                        field_crosses<1, true>(t, key, min_weight, neg) || field_crosses<1, false>(t, key, min_weight, neg) ||
                        field_crosses<2, true>(t, key, min_weight, neg) || field_crosses<2, false>(t, key, min_weight, neg))
                        st |= VISO_FIELD_STATE_SURFACE;
                }
            }
            site = (st & VISO_FIELD_STATE_SURFACE) || (unknown_is_site && !st);
            g[c] = site ? 0u : VISO_FIELD_NONE;
            state[c] = (uint8_t)st;
        }
        sites += (uint32_t)__popcll(__ballot(site));
    }
    if (sites && (threadIdx.x & 63) == 0) atomicAdd(t.head.words + VOXEL_W_OUT, (unsigned long long)sites);
}

// One pass along the axis whose cells lie `stride` words apart and which is n long: in and out are different buffers.
__global__ __launch_bounds__(256) void tsdf_field_pass_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t cells,
                                                              uint32_t stride, uint32_t n) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cells) return;
    const uint32_t i = (c / stride) % n;
    const uint32_t below = i, above = n - 1u - i;            // cells of the line on either side
    const uint32_t reach = below > above ? below : above;    // < n <= 512
    uint32_t best = in[c];
    for (uint32_t d = 1; d <= reach && d * d < best; ++d) {  // (VISO_FIELD_NONE is above every d * d)
        const uint32_t dd = d * d;
        if (d <= below) {
            const uint32_t v = in[c - d * stride];
            if (v != VISO_FIELD_NONE && v + dd < best) best = v + dd;
        }
        if (d <= above) {
            const uint32_t v = in[c + d * stride];
            if (v != VISO_FIELD_NONE && v + dd < best) best = v + dd;
        }
    }
    out[c] = best;
}

bool field_box_arg(const char* where, const viso_voxel_box* box, FieldBox* b) {
    size_t cells = 1;
    for (int i = 0; i < 3; ++i) {
        const long long n = (long long)box->hi[i] - (long long)box->lo[i];
        if (n < 1 || n > FIELD_MAX_AXIS) {
            viso_set_error("%s: bad argument (the box has %lld voxels on axis %d: 1 .. %d)", where, n, i, FIELD_MAX_AXIS);
            return false;
        }
        b->lo[i] = box->lo[i];
        b->n[i] = (uint32_t)n;
        cells *= (size_t)n;
    }
    b->cells = (uint32_t)cells;
    return true;
}

int field_passes(VoxelHost* h, const TsdfTable& t, uint32_t min_weight, const FieldBox& b, uint32_t unknown_is_site, uint32_t* result,
                 uint32_t* other, uint8_t* d_state, unsigned long long* n_sites) {
    const dim3 grid((b.cells + 255u) / 256u);
    const dim3 site_grid(grid.x < FIELD_SITE_BLOCKS ? grid.x : FIELD_SITE_BLOCKS);
    return voxel_pass(h, [&](hipStream_t s) {
        hipLaunchKernelGGL(tsdf_field_sites_kernel, site_grid, dim3(256), 0, s, t, min_weight, b, unknown_is_site, other, d_state);
        hipLaunchKernelGGL(tsdf_field_pass_kernel, grid, dim3(256), 0, s, other, result, b.cells, 1u, b.n[2]);
        hipLaunchKernelGGL(tsdf_field_pass_kernel, grid, dim3(256), 0, s, result, other, b.cells, b.n[2], b.n[1]);
        hipLaunchKernelGGL(tsdf_field_pass_kernel, grid, dim3(256), 0, s, other, result, b.cells, b.n[1] * b.n[2], b.n[0]);
    }, n_sites);
}

extern "C" int viso_tsdf_distance_field(viso_tsdf* t, uint32_t min_weight, const viso_voxel_box* box, uint32_t flags, uint32_t* sq_out,
                                        uint8_t* state_out_or_null, size_t n_cap, size_t* n_sites_or_null) {
    const char* where = "viso_tsdf_distance_field";
    // what does not need the map first, so that nothing of a wrong call reaches a handle
    if (min_weight < 1 || !box || !sq_out || (flags & ~VISO_FIELD_UNKNOWN_IS_SITE)) {
        viso_set_error("%s: bad argument (min_weight >= 1, a non-null box and sq_out, no flag but VISO_FIELD_UNKNOWN_IS_SITE)", where);
        return VISO_ERR_ARG;
    }
    FieldBox b;
    if (!field_box_arg(where, box, &b)) return VISO_ERR_ARG;
    const size_t cells = b.cells;
    if (n_cap < cells) {
        viso_set_error("%s: the %zu cells of the box do not fit the %zu given", where, cells, n_cap);
        return VISO_ERR_ARG;
    }
    VoxelRegistry& reg = tsdf_registry();
    if (!voxel_known(reg, t)) { viso_set_error("%s: not a live TSDF handle", where); return VISO_ERR_ARG; }
    VoxelSession ses(where, reg, t);
    VISO_TRY(ses.status());
    TsdfView v;
    tsdf_view(t, &v);
    VoxelScratch d(ses, cells * (2 * sizeof(uint32_t) + 1), "the field");   // g | g' | state
    VISO_TRY(d.status());
    uint32_t* ga = d.as<uint32_t>();
    uint32_t* gb = ga + cells;
    uint8_t* d_state = reinterpret_cast<uint8_t*>(gb + cells);
    unsigned long long n_sites = 0;
    VISO_TRY(field_passes(ses.host(), v.t, min_weight, b, flags & VISO_FIELD_UNKNOWN_IS_SITE, gb, ga, d_state, &n_sites));
    HIP_TRY(hipMemcpyAsync(sq_out, gb, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, ses.stream()));
    if (state_out_or_null) HIP_TRY(hipMemcpyAsync(state_out_or_null, d_state, cells, hipMemcpyDeviceToHost, ses.stream()));
    VISO_TRY(d.release());
    if (n_sites_or_null) *n_sites_or_null = (size_t)n_sites;
    return VISO_OK;
}
