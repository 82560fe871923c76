// tsdf_travel.hip — the travel field of a TSDF map over a box of voxels (include/viso_hip.h, "TSDF travel field"):
// for every cell of the box the cost of the cheapest sequence of <3,4,5> chamfer moves through free cells to a goal.  Opt-in, NOT in
// the reference.  The definition is the header's; the device output is bit-identical to tests/travel_ref.py.
//
// The distance field first (field_passes of tsdf_field.hip: its kernels, unchanged), then, over the buffer that the passes leave free:
//   tsdf_travel_init_kernel    one thread per cell: TRAVEL_UNREACHED in a free cell, VISO_FIELD_NONE in every other one.  The two
//                              values stay apart until the last kernel, so a cell that is not free is never lowered or stepped from
//   tsdf_travel_goals_kernel   one thread per goal: 0 into a free cell of the box; its tile, and the up to seven more that have the
//                              cell in their halo, onto the list of round 1
//   tsdf_travel_relax_kernel   one launch a round.  A workgroup of 512 threads takes the tiles of the round's list one after the
//                              other: the tile's 8 x 8 x 8 cells and a halo of one cell into LDS (10^3 words), one thread per
//                              cell, sweeps of "the minimum over the 26 neighbours of theirs plus the move's" in LDS until a
//                              sweep lowers nothing, the lowered cells back to memory (its own cells only), and every neighbour
//                              tile whose halo holds a lowered cell onto the next round's list.  A word per tile holds the last
//                              round the tile was listed for, taken with atomicExch: no tile is on a list twice
//   tsdf_travel_finish_kernel  TRAVEL_UNREACHED becomes VISO_FIELD_NONE; the finite cells are counted, one atomic per wave
// Nothing orders workgroups inside a launch.  A tile may read a halo word while its owner lowers it: values only fall, every value
// ever written is the cost of a real sequence of moves, and the owner lists the reader for the next round, whose launch sees all of
// this round's stores.  The fixed point is unique, so the result does not depend on any of that.
// The round's list length stays on the device (three counters in turn: read, appended to, zeroed), so the host looks only every
// TRAVEL_CHECK_EVERY rounds; a launch that finds an empty list does nothing.
// Bounds: a sweep loop ends after at most 513 sweeps (a chain of lowerings inside a tile visits a cell once); a workgroup takes at
// most tiles / gridDim.x + 1 tiles; the other kernels take at most 256 rounds of cells a block; the host launches at most
// cells + 1 rounds.  Device memory of a call: two uint32 and one uint8 a cell, three uint32 a tile, 12 bytes a goal and 8 words.
#include "common.h"
#include "tsdf_field.h"

#define TRAVEL_UNREACHED 0xfffffffeu   // a free cell that no sequence has reached (yet); every finite cost is <= 5 * 2^27
#define TRAVEL_MAX_GOALS 65536
#define TRAVEL_TILE 8
#define TRAVEL_HALO (TRAVEL_TILE + 2)
#define TRAVEL_HALO_WORDS (TRAVEL_HALO * TRAVEL_HALO * TRAVEL_HALO)
#define TRAVEL_SWEEPS 513              // 512 cells a tile, and the sweep that finds nothing to lower
#define TRAVEL_BLOCKS 2048             // the largest grid of a kernel here
#ifndef TRAVEL_CHECK_EVERY
#define TRAVEL_CHECK_EVERY 4           // rounds between two looks of the host at the list's length (DESIGN.md 5.25 has the timings)
#endif
// the call's words on the device
#define TRAVEL_W_COUNT 0               // 0, 1, 2: the list's length of round r at r % 3
#define TRAVEL_W_ROUNDS 3              // the last round that found a list
#define TRAVEL_W_GOALS 4               // goals used
#define TRAVEL_W_REACHED 5             // finite cells
#define TRAVEL_WORDS 8

struct TravelTiles {
    uint32_t nt[3];   // tiles an axis, <= 64
    uint32_t tiles;   // <= 2^18
};

// `tile` onto the list of round `round` unless it is on it: the word of the tile holds the last round it was listed for
__device__ __forceinline__ void travel_queue(uint32_t tile, uint32_t round, const TravelTiles& tt, uint32_t* queued, uint32_t* list,
                                             uint32_t* ctl) {
    if (atomicExch(queued + tile, round) == round) return;
    const uint32_t at = atomicAdd(ctl + TRAVEL_W_COUNT + round % 3u, 1u);
    if (at < tt.tiles) list[at] = tile;   // (always: a tile is listed once a round)
}

// The tiles that hold the cell (l0, l1, l2) of a tile or have it in their halo, one bit each: bit (e0 + 1) 9 + (e1 + 1) 3 + e2 + 1 for
// the tile at +e (bit 13: the cell's own).  The tile at +e sees the cell when, on every axis, e is 0 or the cell is the tile's
// first (e < 0) or last (e > 0) one.
__device__ __forceinline__ uint32_t travel_seen_by(int l0, int l1, int l2) {
    uint32_t m = 0u;
#pragma unroll
    for (int e0 = -1; e0 <= 1; ++e0)
#pragma unroll
        for (int e1 = -1; e1 <= 1; ++e1)
#pragma unroll
            for (int e2 = -1; e2 <= 1; ++e2) {
                const bool sees = (e0 == 0 || l0 == (e0 < 0 ? 0 : TRAVEL_TILE - 1)) && (e1 == 0 || l1 == (e1 < 0 ? 0 : TRAVEL_TILE - 1)) &&
                                  (e2 == 0 || l2 == (e2 < 0 ? 0 : TRAVEL_TILE - 1));
                if (sees) m |= 1u << ((e0 + 1) * 9 + (e1 + 1) * 3 + e2 + 1);
            }
    return m;
}

// the tiles of the bits of `dirs` around the tile (t0, t1, t2), those inside the box, onto the list of round `round`: lane d < 27 of
// the caller takes bit d
__device__ __forceinline__ void travel_queue_around(uint32_t dirs, uint32_t d, int t0, int t1, int t2, uint32_t round, const TravelTiles& tt,
                                                    uint32_t* queued, uint32_t* list, uint32_t* ctl) {
    if (!(dirs >> d & 1u)) return;
    const int n0 = t0 + (int)(d / 9u) - 1, n1 = t1 + (int)(d / 3u % 3u) - 1, n2 = t2 + (int)(d % 3u) - 1;
    if (n0 >= 0 && n0 < (int)tt.nt[0] && n1 >= 0 && n1 < (int)tt.nt[1] && n2 >= 0 && n2 < (int)tt.nt[2])
        travel_queue(((uint32_t)n0 * tt.nt[1] + (uint32_t)n1) * tt.nt[2] + (uint32_t)n2, round, tt, queued, list, ctl);
}

__global__ __launch_bounds__(256) void tsdf_travel_init_kernel(const uint32_t* __restrict__ sq, const uint8_t* __restrict__ state, uint32_t cells,
                                                               uint32_t unknown_is_site, uint32_t clearance_sq, uint32_t* __restrict__ cost) {
    // a block takes 256 cells at a time, the grid's blocks apart: at most 256 times (the host sizes the grid: TRAVEL_BLOCKS)
    for (uint32_t c = blockIdx.x * 256 + threadIdx.x; c < cells; c += gridDim.x * 256) {
        const uint32_t st = state[c];
        const bool site = (st & VISO_FIELD_STATE_SURFACE) || (unknown_is_site && !(st & 3u));
        const bool is_free = (st & 3u) != 2u && !site && sq[c] >= clearance_sq;   // (VISO_FIELD_NONE is at least anything)
        cost[c] = is_free ? TRAVEL_UNREACHED : VISO_FIELD_NONE;
    }
}

__global__ __launch_bounds__(256) void tsdf_travel_goals_kernel(const int32_t* __restrict__ goals, uint32_t n_goals, FieldBox b, TravelTiles tt,
                                                                uint32_t* cost, uint32_t* queued, uint32_t* list, uint32_t* ctl) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    bool used = false;
    if (g < n_goals) {
        const long long i0 = (long long)goals[3 * g] - b.lo[0], i1 = (long long)goals[3 * g + 1] - b.lo[1], i2 = (long long)goals[3 * g + 2] - b.lo[2];
        if (i0 >= 0 && i0 < b.n[0] && i1 >= 0 && i1 < b.n[1] && i2 >= 0 && i2 < b.n[2]) {
            const uint32_t c = ((uint32_t)i0 * b.n[1] + (uint32_t)i1) * b.n[2] + (uint32_t)i2;
            // (another goal's thread may have stored the 0 already: the cell is free all the same)
            if (cost[c] != VISO_FIELD_NONE) {
                used = true;
                cost[c] = 0u;
                // the goal's tile and every tile that has the goal in its halo: nothing else tells them of a cost that no round lowered
                const uint32_t dirs = travel_seen_by((int)i0 % TRAVEL_TILE, (int)i1 % TRAVEL_TILE, (int)i2 % TRAVEL_TILE);
                for (uint32_t d = 0; d < 27u; ++d)
                    travel_queue_around(dirs, d, (int)i0 / TRAVEL_TILE, (int)i1 / TRAVEL_TILE, (int)i2 / TRAVEL_TILE, 1u, tt, queued, list, ctl);
            }
        }
    }
    const uint32_t n = (uint32_t)__popcll(__ballot(used));
    if (n && (threadIdx.x & 63) == 0) atomicAdd(ctl + TRAVEL_W_GOALS, n);
}

__global__ __launch_bounds__(512) void tsdf_travel_relax_kernel(FieldBox b, TravelTiles tt, uint32_t* cost, uint32_t* queued,
                                                                const uint32_t* __restrict__ list_in, uint32_t* __restrict__ list_out, uint32_t* ctl,
                                                                uint32_t round) {
    __shared__ uint32_t s_cost[TRAVEL_HALO_WORDS];
    __shared__ uint32_t s_dirs;   // the bits of travel_seen_by: the tile at +e has a lowered cell in its halo
    const uint32_t tid = threadIdx.x;
    uint32_t count = ctl[TRAVEL_W_COUNT + round % 3u];   // the launch before this one wrote it
    if (count > tt.tiles) count = tt.tiles;              // (never: a tile is listed once a round; the list has that many places)
    if (blockIdx.x == 0 && tid == 0) {
        ctl[TRAVEL_W_COUNT + (round + 2u) % 3u] = 0u;   // round + 2's: the launch before this one has read it, the next one appends
        if (count) ctl[TRAVEL_W_ROUNDS] = round;
    }
    const int l0 = (int)(tid >> 6), l1 = (int)(tid >> 3) & 7, l2 = (int)tid & 7;
    const int at = ((l0 + 1) * TRAVEL_HALO + l1 + 1) * TRAVEL_HALO + l2 + 1;
    // the tiles of the list, the grid's blocks apart: count <= tiles
    for (uint32_t i = blockIdx.x; i < count; i += gridDim.x) {
        const uint32_t tile = list_in[i];
        const int t2 = (int)(tile % tt.nt[2]), t1 = (int)(tile / tt.nt[2] % tt.nt[1]), t0 = (int)(tile / (tt.nt[2] * tt.nt[1]));
        if (tid == 0) s_dirs = 0u;
        for (int l = (int)tid; l < TRAVEL_HALO_WORDS; l += 512) {
            const int c0 = t0 * TRAVEL_TILE + l / (TRAVEL_HALO * TRAVEL_HALO) - 1, c1 = t1 * TRAVEL_TILE + l / TRAVEL_HALO % TRAVEL_HALO - 1,
                      c2 = t2 * TRAVEL_TILE + l % TRAVEL_HALO - 1;
            const bool inside = c0 >= 0 && c0 < (int)b.n[0] && c1 >= 0 && c1 < (int)b.n[1] && c2 >= 0 && c2 < (int)b.n[2];
            s_cost[l] = inside ? cost[((uint32_t)c0 * b.n[1] + (uint32_t)c1) * b.n[2] + (uint32_t)c2] : VISO_FIELD_NONE;
        }
        __syncthreads();
        const uint32_t first = s_cost[at];
        uint32_t mine = first;   // only this thread writes s_cost[at]
        for (int sweep = 0; sweep < TRAVEL_SWEEPS; ++sweep) {
            int lowered = 0;
            if (mine != VISO_FIELD_NONE) {
                uint32_t best = mine;
#pragma unroll
                for (int e0 = -1; e0 <= 1; ++e0)
#pragma unroll
                    for (int e1 = -1; e1 <= 1; ++e1)
#pragma unroll
                        for (int e2 = -1; e2 <= 1; ++e2) {
                            if (!(e0 | e1 | e2)) continue;
                            const uint32_t w = 2u + (uint32_t)((e0 != 0) + (e1 != 0) + (e2 != 0));
                            const uint32_t v = s_cost[at + (e0 * TRAVEL_HALO + e1) * TRAVEL_HALO + e2];
                            if (v < TRAVEL_UNREACHED && v + w < best) best = v + w;
                        }
                if (best < mine) {
                    mine = best;
                    s_cost[at] = best;
                    lowered = 1;
                }
            }
            if (!__syncthreads_or(lowered)) break;   // the same answer in every thread
        }
        if (mine < first) {   // a cell of the box: what lies beyond it was loaded as VISO_FIELD_NONE
            cost[((uint32_t)(t0 * TRAVEL_TILE + l0) * b.n[1] + (uint32_t)(t1 * TRAVEL_TILE + l1)) * b.n[2] + (uint32_t)(t2 * TRAVEL_TILE + l2)] = mine;
            const uint32_t m = travel_seen_by(l0, l1, l2) & ~(1u << 13);   // the neighbour tiles that have this cell in their halo
            if (m) atomicOr(&s_dirs, m);
        }
        __syncthreads();
        if (tid < 27u) travel_queue_around(s_dirs, tid, t0, t1, t2, round + 1u, tt, queued, list_out, ctl);
        __syncthreads();   // s_cost and s_dirs are rewritten next
    }
}

__global__ __launch_bounds__(256) void tsdf_travel_finish_kernel(uint32_t* cost, uint32_t cells, uint32_t* ctl) {
    uint32_t reached = 0;   // of this wave, the same in all its lanes
    for (uint32_t base = blockIdx.x * 256; base < cells; base += gridDim.x * 256) {
        const uint32_t c = base + threadIdx.x;
        bool finite = false;
        if (c < cells) {
            const uint32_t v = cost[c];
            if (v == TRAVEL_UNREACHED) cost[c] = VISO_FIELD_NONE;
            finite = v < TRAVEL_UNREACHED;
        }
        reached += (uint32_t)__popcll(__ballot(finite));
    }
    if (reached && (threadIdx.x & 63) == 0) atomicAdd(ctl + TRAVEL_W_REACHED, reached);
}

extern "C" int viso_tsdf_travel_field(viso_tsdf* t, uint32_t min_weight, const viso_voxel_box* box, uint32_t flags, uint32_t clearance_sq,
                                      const int32_t* goals, size_t n_goals, uint32_t* cost_out, uint32_t* sq_out_or_null,
                                      uint8_t* state_out_or_null, size_t n_cap, size_t* n_goals_used_or_null, size_t* n_reached_or_null,
                                      size_t* n_rounds_or_null) {
    const char* where = "viso_tsdf_travel_field";
    // what does not need the map first, so that nothing of a wrong call reaches a handle
    if (min_weight < 1 || !box) {
        viso_set_error("%s: bad argument (min_weight >= 1, a non-null box)", where);
        return VISO_ERR_ARG;
    }
    FieldBox b;
    if (!field_box_arg(where, box, &b)) return VISO_ERR_ARG;
    if ((flags & ~VISO_FIELD_UNKNOWN_IS_SITE) || clearance_sq == VISO_FIELD_NONE || !goals || !cost_out || n_goals < 1 ||
        n_goals > TRAVEL_MAX_GOALS) {
        viso_set_error("%s: bad argument (no flag but VISO_FIELD_UNKNOWN_IS_SITE, clearance_sq below VISO_FIELD_NONE, non-null goals and "
                       "cost_out, 1 .. %d goals)", where, TRAVEL_MAX_GOALS);
        return VISO_ERR_ARG;
    }
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
    TravelTiles tt;
    for (int i = 0; i < 3; ++i) tt.nt[i] = (b.n[i] + TRAVEL_TILE - 1u) / TRAVEL_TILE;
    tt.tiles = tt.nt[0] * tt.nt[1] * tt.nt[2];
    const size_t state_words = (cells + 3) / 4;
    const size_t words = 2 * cells + state_words + 3 * (size_t)tt.tiles + TRAVEL_WORDS + 3 * n_goals;
    uint32_t ctl[TRAVEL_WORDS] = {0};   // (before the block: copies on the stream write it)
    VoxelScratch d(ses, words * sizeof(uint32_t), "the field");   // sq | cost | state | queued | the call's words | two lists | goals
    VISO_TRY(d.status());
    uint32_t* d_sq = d.as<uint32_t>();
    uint32_t* d_cost = d_sq + cells;
    uint8_t* d_state = reinterpret_cast<uint8_t*>(d_cost + cells);
    uint32_t* d_queued = d_cost + cells + state_words;
    uint32_t* d_ctl = d_queued + tt.tiles;
    uint32_t* d_list[2] = {d_ctl + TRAVEL_WORDS, d_ctl + TRAVEL_WORDS + tt.tiles};
    int32_t* d_goals = reinterpret_cast<int32_t*>(d_list[1] + tt.tiles);
    const uint32_t unknown = flags & VISO_FIELD_UNKNOWN_IS_SITE;
    hipStream_t s = ses.stream();
    unsigned long long n_sites = 0;
    // the distance field; the passes' second buffer then becomes the costs
    VISO_TRY(field_passes(ses.host(), v.t, min_weight, b, unknown, d_sq, d_cost, d_state, &n_sites));
    HIP_TRY(hipMemcpyAsync(d_goals, goals, 3 * n_goals * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_queued, 0, ((size_t)tt.tiles + TRAVEL_WORDS) * sizeof(uint32_t), s));
    const unsigned cell_blocks = (unsigned)((cells + 255) / 256);
    const dim3 cell_grid(cell_blocks < TRAVEL_BLOCKS ? cell_blocks : TRAVEL_BLOCKS);
    const dim3 tile_grid(tt.tiles < TRAVEL_BLOCKS ? tt.tiles : TRAVEL_BLOCKS);
    hipLaunchKernelGGL(tsdf_travel_init_kernel, cell_grid, dim3(256), 0, s, d_sq, d_state, b.cells, unknown, clearance_sq, d_cost);
    hipLaunchKernelGGL(tsdf_travel_goals_kernel, dim3((unsigned)((n_goals + 255) / 256)), dim3(256), 0, s, d_goals, (uint32_t)n_goals, b, tt,
                       d_cost, d_queued, d_list[1], d_ctl);
    HIP_TRY(hipGetLastError());
    // One launch a round, the list of round r in d_list[r & 1]; the host looks at the next list's length every TRAVEL_CHECK_EVERY
    // rounds.  At most cells + 1 rounds: more is an error, never a reason to go on.
    const size_t max_rounds = cells + 1;
    for (size_t round = 1;;) {
        for (int k = 0; k < TRAVEL_CHECK_EVERY && round <= max_rounds; ++k, ++round)
            hipLaunchKernelGGL(tsdf_travel_relax_kernel, tile_grid, dim3(512), 0, s, b, tt, d_cost, d_queued, d_list[round & 1],
                               d_list[(round + 1) & 1], d_ctl, (uint32_t)round);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (!ctl[TRAVEL_W_COUNT + round % 3]) break;   // nothing is listed for the next round
        if (round > max_rounds) {
            VISO_TRY(d.release());
            viso_set_error("%s: the relaxation has not come to rest after %zu rounds, more than the box has cells", where, max_rounds);
            return VISO_ERR_HIP;
        }
    }
    hipLaunchKernelGGL(tsdf_travel_finish_kernel, cell_grid, dim3(256), 0, s, d_cost, b.cells, d_ctl);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctl, d_ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cost_out, d_cost, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (sq_out_or_null) HIP_TRY(hipMemcpyAsync(sq_out_or_null, d_sq, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (state_out_or_null) HIP_TRY(hipMemcpyAsync(state_out_or_null, d_state, cells, hipMemcpyDeviceToHost, s));
    VISO_TRY(d.release());
    if (n_goals_used_or_null) *n_goals_used_or_null = ctl[TRAVEL_W_GOALS];
    if (n_reached_or_null) *n_reached_or_null = ctl[TRAVEL_W_REACHED];
    if (n_rounds_or_null) *n_rounds_or_null = ctl[TRAVEL_W_ROUNDS];
    return VISO_OK;
}
