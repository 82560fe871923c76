// loops.hip — the opt-in loop-closure detection (include/viso_hip.h, "loop closure").  Not in the reference.
//   place signatures   loop_pack_kernel (direct calls: int16 rows -> the matcher's biased u16 rows), place_sig_kernel (a workgroup a
//                      frame: a lane a row, 12 sign projections in registers, the histogram through LDS atomics)
//   scores, candidates place_sums_kernel, place_score_kernel (64 x 64 tiles of min-sums by v_sad_u8), place_cand_kernel (a workgroup a
//                      row: the greedy pick over the sequence sums, a 64-bit key maximum a round)
//   wide match         wide_scan_kernel (128 queries x all targets in tiles of 64, v_sad_u16 from LDS, minima as packed
//                      (sad << 14 | index) words through atomicMin), wide_accept_kernel (ratio, mutual test, rows in query order)
// Everything is integer work whose reductions are minima, maxima and counts: the results do not depend on any order, and two calls
// give the same bytes.  No kernel uses scratch memory (tests/test_loops_cpu.py reads -Rpass-analysis=kernel-resource-usage).
#include "batch.h"
#include "match_dev.h"
#include "solver_dev.h"

#include <math.h>
#include <algorithm>
#include <vector>

#define LOOP_THREADS 256
#define LOOP_MAX_BITS 12
#define PLACE_TILE 64            // place_score_kernel: rows and columns of a tile
#define PLACE_LD (PLACE_TILE + 1)   // dwords of a staged signature chunk's row (one more than the chunk: the columns' reads spread over the banks)
#define PLACE_BLOCK_BYTES ((size_t)16 << 20)    // viso_place_candidates: the rows of raw scores held at a time (n > 2048: more than one group)
#define PLACE_SCORES_MAX ((size_t)1 << 31)      // viso_place_scores: the largest block it hands out
#define WIDE_TQ 128              // wide_scan_kernel: queries of a workgroup, targets of a tile
#define WIDE_TT 64
#define WIDE_LD 68               // dwords of a staged row (64 + one 16-byte slot: ds_read_b128 of 16 rows meets 16 slots)
#define WIDE_IDX_BITS 14         // a key is sad << 14 | index: cap <= 16384, sad saturates at 2^18 - 2 (no key equals WIDE_NONE)
#define WIDE_SAD_MAX 0x3fffeu
#define WIDE_NONE 0xffffffffu

// "these left-image rows": frame f's packed rows at rows + f * row_fs, its row count at n[f * n_fs]; rank (or null: the identity) maps
// an original index to the row's position, frame f's at rank + f * rank_fs
struct RowSrc { const uint16_t* rows; const int* rank; const int* n; size_t row_fs, rank_fs; int n_fs, cap; };
__device__ __forceinline__ int src_count(const RowSrc& s, int f) { const int n = s.n[(size_t)f * s.n_fs]; return n < 0 ? 0 : n > s.cap ? s.cap : n; }

// ---- rows of the direct calls --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOOP_THREADS) void loop_pack_kernel(const int16_t* desc, size_t n_rows, uint32_t* out) {
    const size_t i = (size_t)blockIdx.x * LOOP_THREADS + threadIdx.x;   // dword i of the packed rows: elements 2l, 2l + 1 of row i / 64
    if (i >= n_rows * (VISO_ROW / 2)) return;
    const size_t row = i >> 6;
    const int e = (int)(i & 63) * 2;
    const int16_t* d = desc + row * 121;
    const uint32_t lo = e < 121 ? (uint32_t)(d[e] + VISO_BIAS) : VISO_BIAS, hi = e + 1 < 121 ? (uint32_t)(d[e + 1] + VISO_BIAS) : VISO_BIAS;
    out[i] = lo | (hi << 16);
}

// ---- place signatures ----------------------------------------------------------------------------------------------------------
struct SigArgs { RowSrc src; int f0, bits; const uint32_t* mask; uint8_t* out; };   // mask[k]: bit b set = c[b][k] is +1; out: frame f0's first

__global__ __launch_bounds__(LOOP_THREADS) void place_sig_kernel(SigArgs a) {
    __shared__ uint32_t hist[1 << LOOP_MAX_BITS];
    const int f = a.f0 + (int)blockIdx.x, nb = 1 << a.bits, tid = threadIdx.x;
    for (int i = tid; i < nb; i += LOOP_THREADS) hist[i] = 0;
    __syncthreads();
    const int n = src_count(a.src, f);
    const uint16_t* rows = a.src.rows + (size_t)f * a.src.row_fs;
    for (int r = tid; r < n; r += LOOP_THREADS) {   // a bag: the rows' order (bucket order in a batch) does not matter
        const uint4* p = reinterpret_cast<const uint4*>(rows + (size_t)r * VISO_ROW);
        int acc[LOOP_MAX_BITS];
#pragma unroll
        for (int b = 0; b < LOOP_MAX_BITS; ++b) acc[b] = 0;
#pragma unroll 1
        for (int c = 0; c < VISO_ROW / 8; ++c) {
            const uint4 v = p[c];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int d = (int)((w[e >> 1] >> (16 * (e & 1))) & 0xffffu) - VISO_BIAS;   // the pad elements are 0: no term
                const uint32_t m = a.mask[c * 8 + e];                                       // the same word in every lane
#pragma unroll
                for (int b = 0; b < LOOP_MAX_BITS; ++b) acc[b] += ((m >> b) & 1u) ? d : -d;
            }
        }
        uint32_t word = 0;
#pragma unroll
        for (int b = 0; b < LOOP_MAX_BITS; ++b) word |= (acc[b] > 0 ? 1u : 0u) << b;
        atomicAdd(&hist[word & (uint32_t)(nb - 1)], 1u);
    }
    __syncthreads();
    uint32_t* out = reinterpret_cast<uint32_t*>(a.out + ((size_t)blockIdx.x << a.bits));
    for (int i = tid; i < nb / 4; i += LOOP_THREADS)
        out[i] = min(hist[4 * i], 255u) | (min(hist[4 * i + 1], 255u) << 8) | (min(hist[4 * i + 2], 255u) << 16) | (min(hist[4 * i + 3], 255u) << 24);
}

// ---- scores --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOOP_THREADS) void place_sums_kernel(const uint32_t* sig, int n, int words, uint32_t* sums) {
    const int f = (int)blockIdx.x * (LOOP_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (f >= n) return;   // wave uniform
    uint32_t s = 0;
    for (int w = lane; w < words; w += 64) s = __builtin_amdgcn_sad_u8(sig[(size_t)f * words + w], 0u, s);
    s = viso_wave_scan(s);
    if (lane == 63) sums[f] = s;
}

// out[(j - r0) * ld + i] = s(j, i) for r0 <= j < r1, i <= j; with `upper` also 0 for j < i < ld (viso_place_scores' block)
struct ScoreArgs { const uint32_t* sig; const uint32_t* sums; int words, r0, r1, ld, upper; uint32_t* out; };

__global__ __launch_bounds__(LOOP_THREADS) void place_score_kernel(ScoreArgs a) {
    __shared__ uint32_t A[PLACE_TILE * PLACE_LD], B[PLACE_TILE * PLACE_LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int jb = a.r0 + (int)blockIdx.y * PLACE_TILE, ib = (int)blockIdx.x * PLACE_TILE;
    const int jend = min(jb + PLACE_TILE, a.r1);
    if (!a.upper && ib > jend - 1) return;   // a tile above the diagonal (uniform)
    uint32_t acc[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[p][q] = 0;
    const int cw = min(a.words, PLACE_TILE);   // dwords of a chunk: 16 (bits 6) .. 64
    const int lcw = 31 - __builtin_clz((unsigned)cw);
    for (int w0 = 0; w0 < a.words; w0 += cw) {
        __syncthreads();
        for (int x = tid; x < PLACE_TILE * cw; x += LOOP_THREADS) {
            const int r = x >> lcw, c = x & (cw - 1);
            const int j = jb + r, i = ib + r;
            A[r * PLACE_LD + c] = j < a.r1 ? a.sig[(size_t)j * a.words + w0 + c] : 0u;
            B[r * PLACE_LD + c] = i < a.ld ? a.sig[(size_t)i * a.words + w0 + c] : 0u;
        }
        __syncthreads();
        for (int c = 0; c < cw; ++c) {
            uint32_t hj[4], hi[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) { hj[p] = A[(ty + 16 * p) * PLACE_LD + c]; hi[p] = B[(tx + 16 * p) * PLACE_LD + c]; }
#pragma unroll
            for (int p = 0; p < 4; ++p)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[p][q] = __builtin_amdgcn_sad_u8(hj[p], hi[q], acc[p][q]);
        }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int j = jb + ty + 16 * p;
        if (j >= a.r1) continue;
        const uint32_t sj = a.sums[j];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = ib + tx + 16 * q;
            if (i <= j) a.out[(size_t)(j - a.r0) * a.ld + i] = (sj + a.sums[i] - acc[p][q]) >> 1;   // sum min = (sum + sum - SAD) / 2
            else if (a.upper && i < a.ld) a.out[(size_t)(j - a.r0) * a.ld + i] = 0u;
        }
    }
}

// ---- candidates ----------------------------------------------------------------------------------------------------------------
// s: the raw scores of rows r0 .. (row j's at s + (j - r0) * ld); a workgroup does row ja + blockIdx.x, output row (j - j0)
struct CandArgs { const uint32_t* s; int r0, ld, ja, j0, min_gap, L, nms, k; uint32_t min_score; int32_t* cand; uint32_t* score; };

__global__ __launch_bounds__(LOOP_THREADS) void place_cand_kernel(CandArgs a) {
    __shared__ int pick[16];
    __shared__ unsigned long long red[LOOP_THREADS / 64];
    const int tid = threadIdx.x, j = a.ja + (int)blockIdx.x;
    int32_t* cand = a.cand + (size_t)(j - a.j0) * a.k;
    uint32_t* score = a.score + (size_t)(j - a.j0) * a.k;
    if (tid < a.k) { cand[tid] = -1; score[tid] = 0u; }
    const int hi = j - a.min_gap;   // the admissible i: 0 .. hi
    for (int r = 0; r < a.k; ++r) {
        __syncthreads();   // pick[r - 1], and the fill of the first round
        unsigned long long best = 0;   // S << 32 | ~i: the maximum is the largest S, then the smallest i; 0 = none
        for (int i = tid; i <= hi; i += LOOP_THREADS) {
            bool gone = false;
            for (int p = 0; p < r; ++p) gone = gone || abs(i - pick[p]) <= a.nms;
            if (gone) continue;
            uint32_t S = 0;
            const int terms = min(a.L, i + 1);   // i - k >= 0
            for (int k = 0; k < terms; ++k) S += a.s[(size_t)(j - k - a.r0) * a.ld + (i - k)];
            if (S < a.min_score) continue;
            const unsigned long long key = ((unsigned long long)S << 32) | (0xffffffffu - (uint32_t)i);
            best = key > best ? key : best;
        }
        best = wave_max_u64(best);
        if ((tid & 63) == 0) red[tid >> 6] = best;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < LOOP_THREADS / 64; ++w) best = red[w] > best ? red[w] : best;
        if (best == 0) break;   // uniform: nothing admissible is left
        if (tid == 0) {
            const int i = (int)(0xffffffffu - (uint32_t)best);
            pick[r] = i; cand[r] = i; score[r] = (uint32_t)(best >> 32);
        }
    }
}

// ---- wide match ----------------------------------------------------------------------------------------------------------------
// tbest [np][cap]: per target the least (sad << 14 | q), WIDE_NONE before; qbest [np][cap][2]: per query the two least (sad << 14 | t)
struct WideArgs { RowSrc src; const int* pairs; int np; uint32_t* tbest; uint32_t* qbest; double ratio; int32_t* match; int32_t* m; };

__device__ __forceinline__ void wide_stage(const RowSrc& s, int f, int base, int n, int rows, uint32_t* lds, int tid) {
    const uint16_t* fr = s.rows + (size_t)f * s.row_fs;
    const int* rank = s.rank ? s.rank + (size_t)f * s.rank_fs : nullptr;
    for (int x = tid; x < rows * 16; x += LOOP_THREADS) {   // 16 lanes a row: 256 contiguous bytes
        const int r = x >> 4, c = x & 15, idx = base + r;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (idx < n) v = reinterpret_cast<const uint4*>(fr + (size_t)(rank ? rank[idx] : idx) * VISO_ROW)[c];
        *reinterpret_cast<uint4*>(lds + r * WIDE_LD + c * 4) = v;
    }
}

__global__ __launch_bounds__(LOOP_THREADS) void wide_scan_kernel(WideArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t Q[WIDE_TQ * WIDE_LD];
    __shared__ __attribute__((aligned(16))) uint32_t T[WIDE_TT * WIDE_LD];
    __shared__ uint32_t tmin[WIDE_TT], k1s[WIDE_TQ], k2s[WIDE_TQ];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, pair = blockIdx.y;
    const int fq = a.pairs[2 * pair], ft = a.pairs[2 * pair + 1];
    const int nq = src_count(a.src, fq), nt = src_count(a.src, ft), qb = (int)blockIdx.x * WIDE_TQ;
    if (qb >= nq) return;   // uniform
    wide_stage(a.src, fq, qb, nq, WIDE_TQ, Q, tid);
    if (tid < WIDE_TT) tmin[tid] = WIDE_NONE;
    if (tid < WIDE_TQ) { k1s[tid] = WIDE_NONE; k2s[tid] = WIDE_NONE; }
    uint32_t k1[8], k2[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) k1[p] = k2[p] = WIDE_NONE;
    for (int tb = 0; tb < nt; tb += WIDE_TT) {
        __syncthreads();   // the tile before is read, its minima are flushed
        wide_stage(a.src, ft, tb, nt, WIDE_TT, T, tid);
        __syncthreads();
        uint32_t acc[8][4];
#pragma unroll
        for (int p = 0; p < 8; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[p][q] = 0;
#pragma unroll 2
        for (int c = 0; c < 16; ++c) {
            uint4 tv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) tv[q] = *reinterpret_cast<const uint4*>(T + (tx + 16 * q) * WIDE_LD + c * 4);
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const uint4 qv = *reinterpret_cast<const uint4*>(Q + (ty + 16 * p) * WIDE_LD + c * 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    uint32_t s = acc[p][q];
                    s = __builtin_amdgcn_sad_u16(qv.x, tv[q].x, s);
                    s = __builtin_amdgcn_sad_u16(qv.y, tv[q].y, s);
                    s = __builtin_amdgcn_sad_u16(qv.z, tv[q].z, s);
                    s = __builtin_amdgcn_sad_u16(qv.w, tv[q].w, s);
                    acc[p][q] = s;
                }
            }
        }
        uint32_t tm[4] = {WIDE_NONE, WIDE_NONE, WIDE_NONE, WIDE_NONE};
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int qi = qb + ty + 16 * p;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ti = tb + tx + 16 * q;
                const uint32_t sad = min(acc[p][q], WIDE_SAD_MAX) << WIDE_IDX_BITS;
                const bool ok = qi < nq && ti < nt;
                const uint32_t kq = ok ? sad | (uint32_t)ti : WIDE_NONE, kt = ok ? sad | (uint32_t)qi : WIDE_NONE;
                k2[p] = min(k2[p], max(k1[p], kq));
                k1[p] = min(k1[p], kq);
                tm[q] = min(tm[q], kt);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) if (tm[q] != WIDE_NONE) atomicMin(&tmin[tx + 16 * q], tm[q]);
        __syncthreads();
        if (tid < WIDE_TT) {
            const uint32_t v = tmin[tid];
            tmin[tid] = WIDE_NONE;
            if (v != WIDE_NONE) atomicMin(&a.tbest[(size_t)pair * a.src.cap + tb + tid], v);   // v names a target below nt
        }
    }
    // a query's two least keys over the 16 lanes that share it: keys are distinct (they carry the target), so the least is one lane's
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 8; ++p) if (k1[p] != WIDE_NONE) atomicMin(&k1s[ty + 16 * p], k1[p]);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const uint32_t second = k1[p] == k1s[ty + 16 * p] ? k2[p] : k1[p];
        if (second != WIDE_NONE) atomicMin(&k2s[ty + 16 * p], second);
    }
    __syncthreads();
    if (tid < WIDE_TQ && qb + tid < nq) {
        uint32_t* o = a.qbest + ((size_t)pair * a.src.cap + qb + tid) * 2;
        o[0] = k1s[tid]; o[1] = k2s[tid];
    }
}

__global__ __launch_bounds__(LOOP_THREADS) void wide_accept_kernel(WideArgs a) {
    __shared__ int wsum[LOOP_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pair = blockIdx.x;
    const int fq = a.pairs[2 * pair], ft = a.pairs[2 * pair + 1];
    const int nq = src_count(a.src, fq), nt = src_count(a.src, ft);
    int32_t* out = a.match + (size_t)pair * a.src.cap * 3;
    int base = 0;
    for (int q0 = 0; q0 < nq && nt > 0; q0 += LOOP_THREADS) {
        const int q = q0 + tid;
        bool take = false;
        uint32_t t1 = 0, d1 = 0;
        if (q < nq) {
            const uint32_t* kb = a.qbest + ((size_t)pair * a.src.cap + q) * 2;
            const uint32_t ka = kb[0], kc = kb[1];
            if (ka != WIDE_NONE) {
                t1 = ka & ((1u << WIDE_IDX_BITS) - 1u); d1 = ka >> WIDE_IDX_BITS;
                const double d2 = kc == WIDE_NONE ? __builtin_huge_val() : (double)(kc >> WIDE_IDX_BITS);
                take = (double)d1 < d2 * a.ratio && a.tbest[(size_t)pair * a.src.cap + t1] == ((d1 << WIDE_IDX_BITS) | (uint32_t)q);
            }
        }
        const unsigned long long bal = __ballot(take);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int at = base + mbcnt(bal);
        for (int w = 0; w < wave; ++w) at += wsum[w];
        if (take) { out[3 * at] = q; out[3 * at + 1] = (int)t1; out[3 * at + 2] = (int)d1; }
        for (int w = 0; w < LOOP_THREADS / 64; ++w) base += wsum[w];
        __syncthreads();
    }
    if (tid == 0) a.m[pair] = base;
}

// ---- host: checks that need no device --------------------------------------------------------------------------------------------
static void sign_masks(uint64_t seed, uint32_t* mask /*[128]*/) {
    for (int k = 0; k < VISO_ROW; ++k) mask[k] = 0;
    for (int b = 0; b < LOOP_MAX_BITS; ++b) {
        unsigned long long s = (unsigned long long)seed * 0x9E3779B97F4A7C15ULL + (unsigned long long)b;
        const unsigned long long draw[2] = {viso_splitmix64(&s), viso_splitmix64(&s)};
        for (int k = 0; k < 121; ++k) mask[k] |= (uint32_t)((draw[k >> 6] >> (k & 63)) & 1ULL) << b;
    }
}

static int bad_arg(const char* where, const char* what) { viso_set_error("%s: bad argument (%s)", where, what); return VISO_ERR_ARG; }

static int check_rows(const char* where, const void* desc, const int32_t* n, int nf, int cap) {
    if (nf < 0 || cap < 1 || cap > (1 << WIDE_IDX_BITS)) return bad_arg(where, "nf >= 0, cap in 1..16384");
    if (nf > 0 && (!desc || !n)) return bad_arg(where, "null descriptors or counts");
    for (int f = 0; f < nf; ++f) if (n[f] < 0 || n[f] > cap) return bad_arg(where, "a row count outside 0..cap");
    return VISO_OK;
}

static int check_pairs(const char* where, const int32_t* pairs, int np, int nf, double ratio, const void* match_out, const void* m_out) {
    if (np < 0 || (np > 0 && (!pairs || !match_out || !m_out))) return bad_arg(where, "np >= 0, non-null pairs and outputs");
    if (!(ratio > 0.0 && ratio <= 1.0)) return bad_arg(where, "ratio in (0, 1]");
    for (int p = 0; p < 2 * np; ++p) if (pairs[p] < 0 || pairs[p] >= nf) return bad_arg(where, "a pair names a frame outside the range");
    return VISO_OK;
}

// a scratch block of the call; a block that has to grow beyond the device's free memory is refused, not tried
template <class T> static int loops_scratch(const char* where, DirectCall& dc, ScratchSlot slot, size_t count, T** out) {
    const size_t bytes = sizeof(T) * count;
    if (dc.c->scratch_bytes[slot] < bytes) {
        size_t fr = 0, tot = 0;
        HIP_TRY(hipMemGetInfo(&fr, &tot));
        if (bytes + bytes / 2 > fr + dc.c->scratch_bytes[slot]) {
            viso_set_error("%s: a working block of %zu bytes does not fit the device's free memory (%zu bytes)", where, bytes + bytes / 2, fr);
            return VISO_ERR_NOMEM;
        }
    }
    return dc.scratch(slot, count, out);
}

static unsigned blocks_of(size_t items) { return (unsigned)((items + LOOP_THREADS - 1) / LOOP_THREADS); }

// desc [nf][cap][121] int16 on the host -> packed rows [nf][cap][128] in SLOT_GEN1, staged through SLOT_GEN0 in groups of frames
static int stage_rows(const char* where, DirectCall& dc, const int16_t* desc, int f0, int nf, int cap, uint16_t** rows_out) {
    const size_t frame = (size_t)cap * 121, group = std::max<size_t>(1, ((size_t)64 << 20) / (frame * sizeof(int16_t)));
    int16_t* raw; uint16_t* rows;
    VISO_TRY(loops_scratch(where, dc, SLOT_GEN0, frame * std::min<size_t>(group, (size_t)nf), &raw));
    VISO_TRY(loops_scratch(where, dc, SLOT_GEN1, (size_t)nf * cap * VISO_ROW, &rows));
    for (size_t g = 0; g < (size_t)nf; g += group) {
        const size_t k = std::min(group, (size_t)nf - g), n_rows = k * cap;
        VISO_TRY(dc.up(raw, desc + ((size_t)f0 + g) * frame, k * frame));
        hipLaunchKernelGGL(loop_pack_kernel, dim3(blocks_of(n_rows * (VISO_ROW / 2))), dim3(LOOP_THREADS), 0, dc.s, raw, n_rows,
                           reinterpret_cast<uint32_t*>(rows + g * cap * VISO_ROW));
        HIP_TRY(hipGetLastError());
    }
    *rows_out = rows;
    return VISO_OK;
}

// ---- place signatures: the calls -------------------------------------------------------------------------------------------------
extern "C" int viso_place_signatures(viso_ctx* ctx_or_null, const int16_t* desc, const int32_t* n, int nf, int cap, uint64_t seed, int bits,
                                     uint8_t* sig_out) {
    const char* where = "viso_place_signatures";
    VISO_TRY(check_rows(where, desc, n, nf, cap));
    if (bits < 6 || bits > LOOP_MAX_BITS || (nf > 0 && !sig_out)) return bad_arg(where, "bits in 6..12, a non-null output");
    VISO_TRY(ctx_resolve(where, ctx_or_null, nullptr));
    if (nf == 0) return VISO_OK;
    uint32_t mask[VISO_ROW];
    sign_masks(seed, mask);
    DirectCall dc;
    VISO_TRY(dc.begin(ctx_or_null));
    // SLOT_GEN2: counts [group] | masks [128] | signatures [group][1 << bits]; the frames in groups whose rows fit 256 MiB
    const size_t group = std::min<size_t>((size_t)nf, std::max<size_t>(1, ((size_t)256 << 20) / ((size_t)cap * VISO_ROW * 2)));
    const size_t oM = al256(sizeof(int) * group), oS = al256(oM + sizeof(mask)), bytes = oS + (group << bits);
    char* blk;
    VISO_TRY(loops_scratch(where, dc, SLOT_GEN2, bytes, &blk));
    VISO_TRY(dc.up(blk + oM, mask, VISO_ROW));
    for (size_t g = 0; g < (size_t)nf; g += group) {
        const size_t k = std::min(group, (size_t)nf - g);
        uint16_t* rows;
        VISO_TRY(stage_rows(where, dc, desc, (int)g, (int)k, cap, &rows));
        VISO_TRY(dc.up(blk, n + g, k));
        SigArgs a;
        a.src = RowSrc{rows, nullptr, reinterpret_cast<const int*>(blk), (size_t)cap * VISO_ROW, 0, 1, cap};
        a.f0 = 0; a.bits = bits; a.mask = reinterpret_cast<const uint32_t*>(blk + oM); a.out = reinterpret_cast<uint8_t*>(blk + oS);
        hipLaunchKernelGGL(place_sig_kernel, dim3((unsigned)k), dim3(LOOP_THREADS), 0, dc.s, a);
        HIP_TRY(hipGetLastError());
        VISO_TRY(dc.down(sig_out + (g << bits), blk + oS, k << bits));
        if (g + group < (size_t)nf) VISO_TRY(dc.wait());   // the next group's counts and rows take this one's place
    }
    return dc.wait();
}

// the batch's left-image rows of its last run, for a call named `where`: live, 121 elements, a completed run, no image flagged
static int batch_rows(const char* where, viso_batch* b, RowSrc* src) {
    if (dead(b)) { viso_set_error("%s: not a live batch handle", where); return VISO_ERR_ARG; }
    if (b->dlen != 121 || b->cap > (1 << WIDE_IDX_BITS)) { viso_set_error("%s: needs descriptors of 121 elements and cap <= 16384", where); return VISO_ERR_ARG; }
    if (!b->has_run) { viso_set_error("%s: needs a completed run (viso_batch_run*): the packed rows are a run's", where); return VISO_ERR_ARG; }
    // the counts are the RUN's own (sort_kp_kernel leaves an image's n behind its bucket starts), not b->n, which an upload or a
    // detect since then may have changed: rank and the packed rows are written below the run's counts only
    *src = RowSrc{b->packed, b->rank, b->bstart + VISO_NB, 2 * (size_t)b->cap * VISO_ROW, 2 * (size_t)b->cap, 2 * (VISO_NB + 1), b->cap};
    return VISO_OK;
}
// ... behind the arguments' checks: the frames' flags (rows that did not fit the u16 rows hold nothing to compare)
static int batch_rows_fit(const char* where, viso_batch* b) {
    VISO_TRY(enter(b));
    if (b->desc_i16) return VISO_OK;   // int16 rows always fit
    std::vector<int> flags(2 * (size_t)b->nf);
    HIP_TRY(hipMemcpyAsync(flags.data(), b->bad_img, sizeof(int) * flags.size(), hipMemcpyDeviceToHost, b->ctx->stream));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    for (int t = 0; t < b->nf; ++t)
        if (flags[2 * (size_t)t]) { viso_set_error("%s: frame %d's left descriptors are not integers of 16 bits: no packed rows", where, t); return VISO_ERR_UNSUPPORTED; }
    return VISO_OK;
}

extern "C" int viso_batch_place_signatures(viso_batch* b, int t0, int t1, uint64_t seed, int bits, uint8_t* sig_out) {
    const char* where = "viso_batch_place_signatures";
    RowSrc src;
    VISO_TRY(batch_rows(where, b, &src));
    if (t0 < 0 || t1 < t0 || t1 > b->nf || bits < 6 || bits > LOOP_MAX_BITS || (t1 > t0 && !sig_out))
        return bad_arg(where, "0 <= t0 <= t1 <= n_frames, bits in 6..12, a non-null output");
    if (t1 == t0) return VISO_OK;
    VISO_TRY(batch_rows_fit(where, b));
    uint32_t mask[VISO_ROW];
    sign_masks(seed, mask);
    hipStream_t s = b->ctx->stream;
    const size_t oS = al256(sizeof(mask)), bytes = oS + ((size_t)(t1 - t0) << bits);
    VISO_TRY(b->fit(&b->loop_ws, &b->loop_ws_bytes, bytes, true, where, "loop-closure workspace"));
    HIP_TRY(hipMemcpyAsync(b->loop_ws, mask, sizeof(mask), hipMemcpyHostToDevice, s));
    SigArgs a;
    a.src = src; a.f0 = t0; a.bits = bits; a.mask = reinterpret_cast<const uint32_t*>(b->loop_ws); a.out = reinterpret_cast<uint8_t*>(b->loop_ws + oS);
    hipLaunchKernelGGL(place_sig_kernel, dim3((unsigned)(t1 - t0)), dim3(LOOP_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sig_out, b->loop_ws + oS, (size_t)(t1 - t0) << bits, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VISO_OK;
}

// ---- scores and candidates: the calls --------------------------------------------------------------------------------------------
static int check_sig(const char* where, const uint8_t* sig, int n, int bits, int j0) {
    if (!sig || n < 1 || n > 32768 || bits < 6 || bits > LOOP_MAX_BITS || j0 < 0 || j0 > n)
        return bad_arg(where, "non-null signatures, n in 1..32768, bits in 6..12, j0 in 0..n");
    return VISO_OK;
}

// signatures and their sums on the device: SLOT_GEN0 = sig [n][1 << bits] | sums [n]
static int stage_sig(const char* where, DirectCall& dc, const uint8_t* sig, int n, int bits, const uint32_t** sig_d, const uint32_t** sums_d) {
    const size_t sb = (size_t)n << bits, oU = al256(sb);
    char* blk;
    VISO_TRY(loops_scratch(where, dc, SLOT_GEN0, oU + sizeof(uint32_t) * n, &blk));
    VISO_TRY(dc.up(blk, sig, sb));
    hipLaunchKernelGGL(place_sums_kernel, dim3((unsigned)((n + 3) / 4)), dim3(LOOP_THREADS), 0, dc.s, reinterpret_cast<const uint32_t*>(blk), n,
                       (1 << bits) / 4, reinterpret_cast<uint32_t*>(blk + oU));
    HIP_TRY(hipGetLastError());
    *sig_d = reinterpret_cast<const uint32_t*>(blk); *sums_d = reinterpret_cast<const uint32_t*>(blk + oU);
    return VISO_OK;
}

static int launch_scores(hipStream_t s, const uint32_t* sig, const uint32_t* sums, int bits, int r0, int r1, int ld, bool upper, uint32_t* out) {
    if (r1 <= r0) return VISO_OK;
    ScoreArgs a = {sig, sums, (1 << bits) / 4, r0, r1, ld, upper ? 1 : 0, out};
    const int cols = upper ? ld : r1;
    hipLaunchKernelGGL(place_score_kernel, dim3((unsigned)((cols + PLACE_TILE - 1) / PLACE_TILE), (unsigned)((r1 - r0 + PLACE_TILE - 1) / PLACE_TILE)),
                       dim3(LOOP_THREADS), 0, s, a);
    HIP_TRY(hipGetLastError());
    return VISO_OK;
}

extern "C" int viso_place_scores(viso_ctx* ctx_or_null, const uint8_t* sig, int n, int bits, int j0, uint32_t* s_out) {
    const char* where = "viso_place_scores";
    VISO_TRY(check_sig(where, sig, n, bits, j0));
    if (j0 < n && !s_out) return bad_arg(where, "a null output");
    VISO_TRY(ctx_resolve(where, ctx_or_null, nullptr));
    if (j0 == n) return VISO_OK;
    const size_t cells = (size_t)(n - j0) * n;
    if (cells * sizeof(uint32_t) > PLACE_SCORES_MAX) {
        viso_set_error("%s: a block of %zu bytes is more than this call hands out (%zu): ask for fewer rows (j0)", where, cells * sizeof(uint32_t), PLACE_SCORES_MAX);
        return VISO_ERR_NOMEM;
    }
    DirectCall dc;
    VISO_TRY(dc.begin(ctx_or_null));
    const uint32_t *sig_d, *sums_d;
    VISO_TRY(stage_sig(where, dc, sig, n, bits, &sig_d, &sums_d));
    uint32_t* out;
    VISO_TRY(loops_scratch(where, dc, SLOT_GEN2, cells, &out));
    VISO_TRY(launch_scores(dc.s, sig_d, sums_d, bits, j0, n, n, true, out));
    VISO_TRY(dc.down(s_out, out, cells));
    return dc.wait();
}

extern "C" int viso_place_candidates(viso_ctx* ctx_or_null, const uint8_t* sig, int n, int bits, int j0, int min_gap, int seq_len, int nms,
                                     uint32_t min_score, int k, int32_t* cand_out, uint32_t* score_out) {
    const char* where = "viso_place_candidates";
    VISO_TRY(check_sig(where, sig, n, bits, j0));
    if (min_gap < 1 || seq_len < 1 || seq_len > 16 || nms < 0 || k < 1 || k > 16)
        return bad_arg(where, "min_gap >= 1, seq_len in 1..16, nms >= 0, k in 1..16");
    if (j0 < n && (!cand_out || !score_out)) return bad_arg(where, "a null output");
    VISO_TRY(ctx_resolve(where, ctx_or_null, nullptr));
    if (j0 == n) return VISO_OK;
    DirectCall dc;
    VISO_TRY(dc.begin(ctx_or_null));
    const uint32_t *sig_d, *sums_d;
    VISO_TRY(stage_sig(where, dc, sig, n, bits, &sig_d, &sums_d));
    // the raw scores of `rows` output rows and the seq_len - 1 rows before them at a time (SLOT_GEN2); the outputs in SLOT_GEN1
    const size_t row_bytes = sizeof(uint32_t) * (size_t)n;
    const int rows = (int)std::min<size_t>((size_t)(n - j0), std::max<size_t>(1, PLACE_BLOCK_BYTES / row_bytes));
    uint32_t* blk; char* outs;
    VISO_TRY(loops_scratch(where, dc, SLOT_GEN2, (size_t)(rows + seq_len - 1) * n, &blk));
    const size_t cells = (size_t)(n - j0) * k, oS = al256(sizeof(int32_t) * cells);
    VISO_TRY(loops_scratch(where, dc, SLOT_GEN1, oS + sizeof(uint32_t) * cells, &outs));
    for (int ja = j0; ja < n; ja += rows) {
        const int jb = std::min(n, ja + rows), r0 = std::max(0, ja - (seq_len - 1));
        VISO_TRY(launch_scores(dc.s, sig_d, sums_d, bits, r0, jb, n, false, blk));
        CandArgs a = {blk, r0, n, ja, j0, min_gap, seq_len, nms, k, min_score, reinterpret_cast<int32_t*>(outs), reinterpret_cast<uint32_t*>(outs + oS)};
        hipLaunchKernelGGL(place_cand_kernel, dim3((unsigned)(jb - ja)), dim3(LOOP_THREADS), 0, dc.s, a);
        HIP_TRY(hipGetLastError());
    }
    VISO_TRY(dc.down(cand_out, outs, cells));
    VISO_TRY(dc.down(score_out, outs + oS, cells));
    return dc.wait();
}

// ---- wide match: the calls -------------------------------------------------------------------------------------------------------
// blk: pairs [np][2] | tbest [np][cap] | qbest [np][cap][2] | match [np][cap][3] | m [np]; the pairs are uploaded here
struct WideBlock { size_t oT, oQ, oM, oC, bytes; };
static WideBlock wide_block(int np, int cap) {
    WideBlock w;
    const size_t cells = (size_t)np * cap;
    w.oT = al256(sizeof(int) * 2 * (size_t)np); w.oQ = al256(w.oT + sizeof(uint32_t) * cells); w.oM = al256(w.oQ + sizeof(uint32_t) * 2 * cells);
    w.oC = al256(w.oM + sizeof(int32_t) * 3 * cells); w.bytes = al256(w.oC + sizeof(int32_t) * np);
    return w;
}

static int launch_wide(hipStream_t s, const RowSrc& src, char* blk, const WideBlock& w, const int32_t* pairs, int np, double ratio,
                       int32_t* match_out, int32_t* m_out) {
    const size_t cells = (size_t)np * src.cap;
    HIP_TRY(hipMemcpyAsync(blk, pairs, sizeof(int32_t) * 2 * (size_t)np, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(blk + w.oT, 0xff, sizeof(uint32_t) * cells, s));        // WIDE_NONE
    HIP_TRY(hipMemsetAsync(blk + w.oQ, 0xff, sizeof(uint32_t) * 2 * cells, s));
    HIP_TRY(hipMemsetAsync(blk + w.oM, 0, sizeof(int32_t) * 3 * cells, s));        // the rows behind a pair's count are zeros
    WideArgs a = {src, reinterpret_cast<const int*>(blk), np, reinterpret_cast<uint32_t*>(blk + w.oT), reinterpret_cast<uint32_t*>(blk + w.oQ), ratio,
                  reinterpret_cast<int32_t*>(blk + w.oM), reinterpret_cast<int32_t*>(blk + w.oC)};
    for (int p0 = 0; p0 < np; p0 += 32768) {   // grid.y <= 65535
        WideArgs c = a;
        const int k = std::min(np - p0, 32768);
        c.pairs += 2 * (size_t)p0; c.tbest += (size_t)p0 * src.cap; c.qbest += 2 * (size_t)p0 * src.cap; c.match += 3 * (size_t)p0 * src.cap; c.m += p0;
        hipLaunchKernelGGL(wide_scan_kernel, dim3((unsigned)((src.cap + WIDE_TQ - 1) / WIDE_TQ), (unsigned)k), dim3(LOOP_THREADS), 0, s, c);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(wide_accept_kernel, dim3((unsigned)k), dim3(LOOP_THREADS), 0, s, c);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(match_out, blk + w.oM, sizeof(int32_t) * 3 * cells, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(m_out, blk + w.oC, sizeof(int32_t) * (size_t)np, hipMemcpyDeviceToHost, s));
    return VISO_OK;
}

extern "C" int viso_wide_match(viso_ctx* ctx_or_null, const int16_t* desc, const int32_t* n, int nf, int cap, const int32_t* pairs, int np,
                               double ratio, int32_t* match_out, int32_t* m_out) {
    const char* where = "viso_wide_match";
    VISO_TRY(check_rows(where, desc, n, nf, cap));
    VISO_TRY(check_pairs(where, pairs, np, nf, ratio, match_out, m_out));
    VISO_TRY(ctx_resolve(where, ctx_or_null, nullptr));
    if (np == 0) return VISO_OK;
    DirectCall dc;
    VISO_TRY(dc.begin(ctx_or_null));
    uint16_t* rows;
    VISO_TRY(stage_rows(where, dc, desc, 0, nf, cap, &rows));
    const WideBlock w = wide_block(np, cap);
    const size_t oN = w.bytes;   // the counts behind the block
    char* blk;
    VISO_TRY(loops_scratch(where, dc, SLOT_GEN2, oN + sizeof(int) * (size_t)nf, &blk));
    VISO_TRY(dc.up(blk + oN, n, (size_t)nf));
    const RowSrc src = {rows, nullptr, reinterpret_cast<const int*>(blk + oN), (size_t)cap * VISO_ROW, 0, 1, cap};
    VISO_TRY(launch_wide(dc.s, src, blk, w, pairs, np, ratio, match_out, m_out));
    return dc.wait();
}

extern "C" int viso_batch_wide_match(viso_batch* b, const int32_t* pairs, int np, double ratio, int32_t* match_out, int32_t* m_out) {
    const char* where = "viso_batch_wide_match";
    RowSrc src;
    VISO_TRY(batch_rows(where, b, &src));
    VISO_TRY(check_pairs(where, pairs, np, b->nf, ratio, match_out, m_out));
    if (np == 0) return VISO_OK;
    VISO_TRY(batch_rows_fit(where, b));
    const WideBlock w = wide_block(np, b->cap);
    VISO_TRY(b->fit(&b->loop_ws, &b->loop_ws_bytes, w.bytes, true, where, "loop-closure workspace"));
    VISO_TRY(launch_wide(b->ctx->stream, src, b->loop_ws, w, pairs, np, ratio, match_out, m_out));
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    return VISO_OK;
}
