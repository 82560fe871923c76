// wave.h — the kernels' cross-lane vocabulary (gfx950, wave64; device only): the lane moves, the wave reductions and scans
// built from them, and the one-instruction helpers that need a source modifier or must not be canonicalised.  Every cross-lane
// builtin and every such inline-asm mnemonic of the library is spelled here and nowhere else (tests/test_wave_header_cpu.py);
// what is about matching rather than about lanes (buckets, qlane, l1_bits) is in match_dev.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- lane moves -------------------------------------------------------------------------------------------------------------
// DPP controls in use: 0xB1 / 0x4E quad_perm [1,0,3,2] / [2,3,0,1] (lane ^ 1 / lane ^ 2), 0x00 / 0x55 / 0xAA / 0xFF quad
// broadcast of lane 0..3, 0x101 row_shl:1, 0x111..0x118 row_shr:1..8, 0x128 row_ror:8 (lane ^ 8), 0x130 / 0x138 wave_shl:1 /
// wave_shr:1, 0x140 row_mirror (15 - lane within 16), 0x141 row_half_mirror (7 - lane within 8), 0x142 / 0x143 row_bcast:15 / :31.
// One function per argument pattern of the builtin:
// old = 0, kept: a lane without a source gets 0 (every lane has one under the quad, mirror and rotate controls)
template <int CTRL>
__device__ __forceinline__ uint32_t wave_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
// old = 0 with bound_ctrl: the same values; for a quad broadcast (every lane has a source: no old value to keep) and the shifts
// whose end lanes take 0, bound_ctrl spares the compiler the old value's initialisation
template <int CTRL>
__device__ __forceinline__ uint32_t wave_dpp_bc(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
// old = the operation's identity, and a row mask: lanes without a source, and the rows outside ROWMASK, take `ident`
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t viso_dpp(uint32_t v, uint32_t ident) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)ident, (int)v, CTRL, ROWMASK, 0xf, false);
}
// lane i <- lane i - 1 / lane i + 1 of the whole wave (gfx9 DPP wave_shr:1 / wave_shl:1); the end lanes get 0
__device__ __forceinline__ float wave_shr1(float v) { return __uint_as_float(wave_dpp_bc<0x138>(__float_as_uint(v))); }
__device__ __forceinline__ float wave_shl1(float v) { return __uint_as_float(wave_dpp_bc<0x130>(__float_as_uint(v))); }
// ds_swizzle, bitmask mode (per 32 lanes): lane' = ((lane & and) | or) ^ xor, PAT = xor << 10 | or << 5 | and.
// 0x101F: lane ^ 4, 0x401F: lane ^ 16 -- the exchanges DPP has no control for
template <int PAT>
__device__ __forceinline__ uint32_t wave_swizzle(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, PAT);
}
// a float of lane k (compile-time constant or wave uniform) as a scalar
__device__ __forceinline__ float readlane_f32(float v, int k) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}
// the same moves of a double: its halves as two 32-bit moves
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double v) {   // lanes without a source, rows outside ROW_MASK: 0.0
    const int lo = (int)viso_dpp<CTRL, ROW_MASK>((uint32_t)__double2loint(v), 0u);
    const int hi = (int)viso_dpp<CTRL, ROW_MASK>((uint32_t)__double2hiint(v), 0u);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double rdlane(double v, int src_lane) {   // src_lane: compile-time constant
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
    return __hiloint2double(hi, lo);
}
template <int I>
__device__ __forceinline__ double swz_bcast8(double v) {   // element I of the lane's aligned group of 8 lanes
    constexpr int pat = (I << 5) | 0x18;                   // bitmask mode: lane' = (lane & 0x18) | I  (per 32 lanes)
    const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), pat);
    const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), pat);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double bperm(double v, int src_lane) {   // any lane's value: the one move here that is an LDS round trip
    const int lo = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2hiint(v));
    return __hiloint2double(hi, lo);
}
// A wave-uniform double into scalar registers (the compiler cannot know a value that came back from LDS or from a
// cross-lane read is uniform): v_readfirstlane of both halves.
__device__ __forceinline__ double uni(double v) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// ---- source modifiers, and min / max as the hardware does them ---------------------------------------------------------------
// |a| + |b|: the absolute values ride on the add as source modifiers -- left to the compiler two neighbouring differences are
// packed and the abs becomes two v_and
__device__ __forceinline__ float abs_add_abs(float a, float b) { float d; asm("v_add_f32_e64 %0, |%1|, |%2|" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ float add_abs_abs(float acc, float a, float b) {   // acc + |a| + |b|
    float d;
    asm("v_add_f32_e64 %0, %1, |%2|\n\tv_add_f32_e64 %0, %0, |%3|" : "=&v"(d) : "v"(acc), "v"(a), "v"(b));
    return d;
}
// fminf / fmaxf without the canonicalising v_max x, x the compiler puts in front (v_min / v_max return the other operand
// for a NaN, like fminf / fmaxf)
__device__ __forceinline__ float fmin_raw(float a, float b) { float r; asm("v_min_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float fmax_raw(float a, float b) { float r; asm("v_max_f32_e32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
// the median of three (for a <= b: the second smallest of a, b, c -- the packed-key trackers' update)
__device__ __forceinline__ uint32_t med3_u32(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// ---- reductions and scans -----------------------------------------------------------------------------------------------------
// Wave-wide steps as DPP operands (row_shr 1, 2, 4, 8 inside the rows of 16 lanes, then row_bcast:15 / :31): the total -- or the
// inclusive prefix -- is in lane 63 after six dependent VALU instructions, where six ds_bpermute round trips (__shfl_xor /
// __shfl_up) take about ten times as long.  The per-image, per-tile and per-problem kernels are chains of such steps between
// their loads; in the latency-bound ones (match_stereo_kernel, the sorts) and for ONE frame (the per-call path) those chains
// are the kernel's duration.  Lanes without a source take the identity.
#define VISO_WAVE_STEPS(OP) OP(0x111, 0xf); OP(0x112, 0xf); OP(0x114, 0xf); OP(0x118, 0xf); OP(0x142, 0xa); OP(0x143, 0xc)
__device__ __forceinline__ uint32_t viso_wave_min63(uint32_t v) {   // valid in lane 63
#define OP_(C, M) v = min(v, viso_dpp<C, M>(v, 0xffffffffu))
    VISO_WAVE_STEPS(OP_);
#undef OP_
    return v;
}
__device__ __forceinline__ uint32_t viso_wave_max63(uint32_t v) {   // valid in lane 63
#define OP_(C, M) v = max(v, viso_dpp<C, M>(v, 0u))
    VISO_WAVE_STEPS(OP_);
#undef OP_
    return v;
}
__device__ __forceinline__ uint32_t viso_wave_scan(uint32_t v) {    // inclusive prefix sum (lane 63: the total)
#define OP_(C, M) v += viso_dpp<C, M>(v, 0u)
    VISO_WAVE_STEPS(OP_);
#undef OP_
    return v;
}
__device__ __forceinline__ unsigned long long viso_wave_sum63(unsigned long long v) {   // valid in lane 63
#define OP_(C, M) v += ((unsigned long long)viso_dpp<C, M>((uint32_t)(v >> 32), 0u) << 32) | viso_dpp<C, M>((uint32_t)v, 0u)
    VISO_WAVE_STEPS(OP_);
#undef OP_
    return v;
}
__device__ __forceinline__ unsigned long long viso_wave_max63(unsigned long long v) {   // valid in lane 63
#define OP_(C, M) do { const unsigned long long o_ = ((unsigned long long)viso_dpp<C, M>((uint32_t)(v >> 32), 0u) << 32) | viso_dpp<C, M>((uint32_t)v, 0u); v = o_ > v ? o_ : v; } while (0)
    VISO_WAVE_STEPS(OP_);
#undef OP_
    return v;
}
__device__ __forceinline__ float viso_wave_fsum63(float v) {        // valid in lane 63 (the order of the additions is this function's)
#define OP_(C, M) v += __uint_as_float(viso_dpp<C, M>(__float_as_uint(v), 0u))
    VISO_WAVE_STEPS(OP_);
#undef OP_
    return v;
}
// Sum of a double over the wave, valid in lane 63: the same six steps (gfx9 reduction idiom; the halves of the double move as
// two 32-bit DPP moves).
__device__ __forceinline__ double wave_sum_to_lane63(double v) {
#define OP_(C, M) v += dpp_f64<C, M>(v)
    VISO_WAVE_STEPS(OP_);
#undef OP_
    return v;
}
// minimum / maximum of a float over the wave, to EVERY lane: quad, half-row and row exchanges as DPP operands, then the four rows'
// values as scalars (fminf / fmaxf ignore a NaN operand: the same result as any other order of the same operations)
template <bool MAX>
__device__ __forceinline__ float viso_wave_fext(float v) {
#define OP_(C) do { const float o_ = __uint_as_float(viso_dpp<C, 0xf>(__float_as_uint(v), 0u)); v = MAX ? fmaxf(v, o_) : fminf(v, o_); } while (0)
    OP_(0xB1); OP_(0x4E); OP_(0x141); OP_(0x140);   // quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
#undef OP_
    const float a = readlane_f32(v, 0), b = readlane_f32(v, 16), c = readlane_f32(v, 32), d = readlane_f32(v, 48);
    return MAX ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : fminf(fminf(a, b), fminf(c, d));
}
// sum over every aligned group of LANES (4 or 8) lanes, to each lane of the group
template <int LANES>
__device__ __forceinline__ uint32_t group_sum(uint32_t v) {
    static_assert(LANES == 4 || LANES == 8, "quad exchanges, then one half-row mirror");
    v += wave_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
    v += wave_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
    if (LANES == 8) v += wave_dpp<0x141>(v);   // row_half_mirror (quads are uniform by now)
    return v;
}
// minimum of a u32 over every row of 16 lanes, to each lane of the row: quad and mirror exchanges
__device__ __forceinline__ uint32_t row_min_u32(uint32_t v) {
    v = min(v, viso_dpp<0xB1, 0xf>(v, 0xffffffffu));    // quad_perm 1,0,3,2
    v = min(v, viso_dpp<0x4E, 0xf>(v, 0xffffffffu));    // quad_perm 2,3,0,1
    v = min(v, viso_dpp<0x141, 0xf>(v, 0xffffffffu));   // row_half_mirror
    v = min(v, viso_dpp<0x140, 0xf>(v, 0xffffffffu));   // row_mirror
    return v;
}
// minimum of a u32 over the wave, to every lane as a scalar.  Not viso_wave_min63 + readlane: this one reduces the rows by the
// exchanges of row_min_u32 where that one uses row_shr steps -- the same value by another instruction sequence, so both stay
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = row_min_u32(v);
    v = min(v, viso_dpp<0x142, 0xa>(v, 0xffffffffu));   // row_bcast:15
    v = min(v, viso_dpp<0x143, 0xc>(v, 0xffffffffu));   // row_bcast:31
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// max over the wave of a u32, to every lane as a scalar: DPP row shifts inside the 16-lane rows, two row broadcasts, the
// total lands in lane 63 (gfx9 reduction idiom; six DPP steps + a readlane instead of six ds_bpermute round trips).  Not
// viso_wave_max63 + readlane: a lane without a source keeps ITS OWN value here (old = v) where that one takes the identity 0 --
// the same value, but the compiler builds each step differently (HISTORY.md), so both stay
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#define OP_(C, M) v = max(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, C, M, 0xf, false))
    VISO_WAVE_STEPS(OP_);   // lane 15 of every row = the row's max after four steps, lane 63 = the wave's after six
#undef OP_
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// max over the wave of a u64 key, to every lane: the high words first, then the low words of the lanes that hold the maximal
// high word (two wave_max_u32 where viso_wave_max63's u64 form compares 64-bit values at every step)
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    const uint32_t mh = wave_max_u32(hi);
    const uint32_t ml = wave_max_u32(hi == mh ? lo : 0u);
    return ((unsigned long long)mh << 32) | ml;
}
