// Test-only harness of the device helper headers (tests/dev_harness.py builds it with the library's own flags; tests/
// test_gpu_dev_helpers.py calls it).  It includes the real headers and copies no helper: every helper, or small group, is wrapped
// in a trivial kernel and an extern "C" host function that takes HOST pointers (allocate, copy, launch, copy back, free) and returns
// the HIP error code (-1: a bad argument).  Whole waves only, as the headers demand: workgroups of 256 threads (four waves), one
// thread per element, n a multiple of 256, every lane active at every call.  Every kernel indexes only its own buffers by thread
// id; the probe loops under test are bounded by construction (voxel_hash.h).
#include "wave.h"
#include "match_dev.h"
#include "voxel_hash.h"
#include "solver_dev.h"

namespace {
struct Dev {   // a device copy of a host array
    void* p = nullptr;
    size_t bytes;
    hipError_t e = hipSuccess;
    Dev(const void* host, size_t b) : bytes(b) {
        if (!b) return;
        e = hipMalloc(&p, b);
        if (e == hipSuccess && host) e = hipMemcpy(p, host, b, hipMemcpyHostToDevice);
    }
    hipError_t back(void* host) const { return bytes ? hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    ~Dev() { if (p) (void)hipFree(p); }
    Dev(const Dev&) = delete;
};
int finish() {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return (int)e;
}

template <class TA, class TB, class TC, class TO>
int dh_run(void (*kern)(const TA*, const TB*, const TC*, TO*, int), const void* a, int sa, const void* b, int sb, const void* c, int sc,
           void* out, int so, int n, int p) {
    if (n <= 0 || n % 256 || !out) return -1;
    Dev da(a, sizeof(TA) * sa * n), db(b, sizeof(TB) * sb * n), dc(c, sizeof(TC) * sc * n), dout(out, sizeof(TO) * so * n);
    if (da.e || db.e || dc.e || dout.e) return (int)(da.e ? da.e : db.e ? db.e : dc.e ? dc.e : dout.e);
    hipLaunchKernelGGL(kern, dim3(n / 256), dim3(256), 0, 0, (const TA*)da.p, (const TB*)db.p, (const TC*)dc.p, (TO*)dout.p, p);
    if (int e = finish()) return e;
    return (int)dout.back(out);
}
}   // namespace

// One thread per element: a, b, c point at the thread's SA / SB / SC input elements, out at its SO outputs; p is a launch-wide int.
// dh_<NAME>(a, b, c, out, n, p) on host arrays; an input with S = 0 is not read (pass null).
#define DH_KERNEL(...) DH_KERNEL_(__VA_ARGS__)   /* (NONE expands to two arguments first) */
#define DH_KERNEL_(NAME, TA, SA, TB, SB, TC, SC, TO, SO, ...)                                                                       \
    __global__ __launch_bounds__(256) void k_##NAME(const TA* A_, const TB* B_, const TC* C_, TO* OUT_, int p) {                   \
        const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;                                                     \
        const TA* a = A_ + (size_t)i * SA; const TB* b = B_ + (size_t)i * SB; const TC* c = C_ + (size_t)i * SC;                    \
        TO* out = OUT_ + (size_t)i * SO;                                                                                            \
        (void)lane; (void)p; (void)a; (void)b; (void)c;                                                                             \
        __VA_ARGS__                                                                                                                 \
    }                                                                                                                               \
    extern "C" int dh_##NAME(const void* a, const void* b, const void* c, void* out, int n, int p) {                               \
        return dh_run<TA, TB, TC, TO>(k_##NAME, a, SA, b, SB, c, SC, out, SO, n, p);                                                \
    }
#define NONE int, 0
typedef unsigned long long u64;

// ---- wave.h: lane moves ---------------------------------------------------------------------------------------------------------
#define DH_WAVE_DPP(C) DH_KERNEL(wave_dpp_##C, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = wave_dpp<C>(a[0]);)
#define DH_WAVE_DPP_BC(C) DH_KERNEL(wave_dpp_bc_##C, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = wave_dpp_bc<C>(a[0]);)
#define DH_VISO_DPP(C, M) DH_KERNEL(viso_dpp_##C##_##M, uint32_t, 1, uint32_t, 1, NONE, uint32_t, 1, out[0] = viso_dpp<C, M>(a[0], b[0]);)
#define DH_DPP_F64(C, M) DH_KERNEL(dpp_f64_##C##_##M, double, 1, NONE, NONE, double, 1, out[0] = dpp_f64<C, M>(a[0]);)
DH_WAVE_DPP(0xB1) DH_WAVE_DPP(0x4E) DH_WAVE_DPP(0x141) DH_WAVE_DPP(0x140) DH_WAVE_DPP(0x128)
DH_WAVE_DPP_BC(0x00) DH_WAVE_DPP_BC(0x55) DH_WAVE_DPP_BC(0xAA) DH_WAVE_DPP_BC(0xFF) DH_WAVE_DPP_BC(0x101) DH_WAVE_DPP_BC(0x130) DH_WAVE_DPP_BC(0x138)
DH_VISO_DPP(0x111, 0xf) DH_VISO_DPP(0x112, 0xf) DH_VISO_DPP(0x114, 0xf) DH_VISO_DPP(0x118, 0xf) DH_VISO_DPP(0x142, 0xa) DH_VISO_DPP(0x143, 0xc)
DH_VISO_DPP(0xB1, 0xf) DH_VISO_DPP(0x4E, 0xf) DH_VISO_DPP(0x141, 0xf) DH_VISO_DPP(0x140, 0xf) DH_VISO_DPP(0x130, 0xf) DH_VISO_DPP(0x138, 0xf)
DH_DPP_F64(0x111, 0xf) DH_DPP_F64(0x112, 0xf) DH_DPP_F64(0x114, 0xf) DH_DPP_F64(0x118, 0xf) DH_DPP_F64(0x142, 0xa) DH_DPP_F64(0x143, 0xc)
DH_KERNEL(wave_shr1, float, 1, NONE, NONE, float, 1, out[0] = wave_shr1(a[0]);)
DH_KERNEL(wave_shl1, float, 1, NONE, NONE, float, 1, out[0] = wave_shl1(a[0]);)
DH_KERNEL(wave_swizzle_0x101F, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = wave_swizzle<0x101F>(a[0]);)
DH_KERNEL(wave_swizzle_0x401F, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = wave_swizzle<0x401F>(a[0]);)
DH_KERNEL(swz_bcast8, double, 1, NONE, NONE, double, 8,
          out[0] = swz_bcast8<0>(a[0]); out[1] = swz_bcast8<1>(a[0]); out[2] = swz_bcast8<2>(a[0]); out[3] = swz_bcast8<3>(a[0]);
          out[4] = swz_bcast8<4>(a[0]); out[5] = swz_bcast8<5>(a[0]); out[6] = swz_bcast8<6>(a[0]); out[7] = swz_bcast8<7>(a[0]);)
DH_KERNEL(bperm, double, 1, int, 1, NONE, double, 1, out[0] = bperm(a[0], b[0]);)
DH_KERNEL(rdlane, double, 1, NONE, NONE, double, 8,   // the source lane is a compile-time constant
          out[0] = rdlane(a[0], 0); out[1] = rdlane(a[0], 15); out[2] = rdlane(a[0], 16); out[3] = rdlane(a[0], 31);
          out[4] = rdlane(a[0], 32); out[5] = rdlane(a[0], 47); out[6] = rdlane(a[0], 48); out[7] = rdlane(a[0], 63);)
DH_KERNEL(readlane_f32, float, 1, int, 1, NONE, float, 1,   // k: uniform over the wave (the wave's first lane's b)
          out[0] = readlane_f32(a[0], __builtin_amdgcn_readfirstlane(b[0]));)
DH_KERNEL(uni, double, 1, NONE, NONE, double, 1, out[0] = uni(a[0]);)

// ---- wave.h: reductions and scans -----------------------------------------------------------------------------------------------
DH_KERNEL(wave_min63, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = viso_wave_min63(a[0]);)
DH_KERNEL(wave_max63, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = viso_wave_max63(a[0]);)
DH_KERNEL(wave_max63_u64, u64, 1, NONE, NONE, u64, 1, out[0] = viso_wave_max63(a[0]);)
DH_KERNEL(wave_scan, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = viso_wave_scan(a[0]);)
DH_KERNEL(wave_sum63, u64, 1, NONE, NONE, u64, 1, out[0] = viso_wave_sum63(a[0]);)
DH_KERNEL(wave_min_u32, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = wave_min_u32(a[0]);)
DH_KERNEL(wave_max_u32, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = wave_max_u32(a[0]);)
DH_KERNEL(wave_max_u64, u64, 1, NONE, NONE, u64, 1, out[0] = wave_max_u64(a[0]);)
DH_KERNEL(row_min_u32, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = row_min_u32(a[0]);)
DH_KERNEL(group_sum_4, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = group_sum<4>(a[0]);)
DH_KERNEL(group_sum_8, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = group_sum<8>(a[0]);)
DH_KERNEL(wave_fext_min, float, 1, NONE, NONE, float, 1, out[0] = viso_wave_fext<false>(a[0]);)
DH_KERNEL(wave_fext_max, float, 1, NONE, NONE, float, 1, out[0] = viso_wave_fext<true>(a[0]);)
DH_KERNEL(wave_fsum63, float, 1, NONE, NONE, float, 1, out[0] = viso_wave_fsum63(a[0]);)
DH_KERNEL(wave_sum_to_lane63, double, 1, NONE, NONE, double, 1, out[0] = wave_sum_to_lane63(a[0]);)
// block_sum<NS, 4>: the thread's NS values in, tot[0..NS) out (every thread returns with tot[] valid)
#define DH_BLOCK_SUM(NS)                                                                                                           \
    DH_KERNEL(block_sum_##NS##_4, double, NS, NONE, NONE, double, NS, __shared__ double red[4 * NS]; __shared__ double tot[NS];      \
              double acc[NS]; for (int k = 0; k < NS; ++k) acc[k] = a[k]; block_sum<NS, 4>(acc, red, tot);                          \
              for (int k = 0; k < NS; ++k) out[k] = tot[k];)
DH_BLOCK_SUM(7) DH_BLOCK_SUM(27) DH_BLOCK_SUM(50)

// ---- wave.h: one-instruction helpers --------------------------------------------------------------------------------------------
DH_KERNEL(abs_add_abs, float, 1, float, 1, NONE, float, 1, out[0] = abs_add_abs(a[0], b[0]);)
DH_KERNEL(add_abs_abs, float, 1, float, 1, float, 1, float, 1, out[0] = add_abs_abs(a[0], b[0], c[0]);)
DH_KERNEL(fmin_raw, float, 1, float, 1, NONE, float, 1, out[0] = fmin_raw(a[0], b[0]);)
DH_KERNEL(fmax_raw, float, 1, float, 1, NONE, float, 1, out[0] = fmax_raw(a[0], b[0]);)
DH_KERNEL(med3_u32, uint32_t, 1, uint32_t, 1, uint32_t, 1, uint32_t, 1, out[0] = med3_u32(a[0], b[0], c[0]);)

// ---- match_dev.h ----------------------------------------------------------------------------------------------------------------
DH_KERNEL(row8_of, int, 1, int, 1, NONE, uint32_t, 1, out[0] = row8_of(a[0], b[0]);)
DH_KERNEL(row8_of_uniform, int, 1, NONE, NONE, uint32_t, 1, out[0] = row8_of_uniform(a[0], p);)            // p: the shift
DH_KERNEL(row8_pair_of_biased, uint32_t, 1, NONE, NONE, uint32_t, 1, out[0] = row8_pair_of_biased(a[0], p);)
DH_KERNEL(pack_block_sums, int, 1, NONE, NONE, uint32_t, 2, const uint2 r = pack_block_sums(a[0]); out[0] = r.x; out[1] = r.y;)
DH_KERNEL(mbcnt, u64, 1, NONE, NONE, int, 1, out[0] = mbcnt(a[0]);)
DH_KERNEL(l1, float, 4, NONE, NONE, uint32_t, 2,   // (qx, qy, tx, ty) -> l1_bits, the bits of l1_kp
          out[0] = l1_bits(a[0], a[1], make_float2(a[2], a[3])); out[1] = __float_as_uint(l1_kp(a[0], a[1], make_float2(a[2], a[3])));)
// (x, x0, scale, w) -> bucket_of, bucket_cvt, and bucket_of_finite where w != 0 (else -1); p: NB (VISO_NB, or the 64 of ST_NBY and MU_NBY)
template <int NB>
__device__ __forceinline__ void dh_buckets(const float* a, int* out) {
    out[0] = bucket_of<NB>(a[0], a[1], a[2]);
    out[1] = bucket_cvt<NB>(a[0], a[1], a[2]);
    out[2] = a[3] != 0.f ? bucket_of_finite<NB>(a[0], a[1], a[2]) : -1;
}
DH_KERNEL(buckets, float, 4, NONE, NONE, int, 3, if (p == VISO_NB) dh_buckets<VISO_NB>(a, out); else dh_buckets<64>(a, out);)
DH_KERNEL(sampson, double, 9, float, 4, NONE, double, 1, out[0] = sampson_dev(a, b[0], b[1], b[2], b[3]);)
DH_KERNEL(epipolar_band, double, 10, float, 5, NONE, float, 1,   // F[9], thresh | xa, xb, ya, yb, r
          out[0] = epipolar_band(a, a[9], b[0], b[1], b[2], b[3], b[4]);)

// One wave per row; the wave of index w writes row 2 w + 1 of buf (rows of VISO_ROW8 bytes): every other row stays a guard.
// mode 0: store_row8_pair (va: the lane's two bytes, h2), 1 / 2: store_row8<false / true> of the elements (va, vb) at shift s.
__global__ __launch_bounds__(256) void k_store_row8(uint8_t* buf, const int* va, const int* vb, int s, int mode) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const size_t row = 2 * (size_t)(i >> 6) + 1;
    const int x = va[i], y = vb[i];
    if (mode == 0) store_row8_pair(buf, row, lane, (uint32_t)x);
    else if (mode == 1) store_row8<false>(buf, row, lane, x, y, s);
    else store_row8<true>(buf, row, lane, x, y, s);
}
extern "C" int dh_store_row8(uint8_t* buf, const int* va, const int* vb, int n, int s, int mode) {   // buf: (2 n / 64 + 1) rows, in and out
    if (n <= 0 || n % 256 || s < 0 || s > 3 || mode < 0 || mode > 2) return -1;
    Dev db(buf, (size_t)(2 * (n / 64) + 1) * VISO_ROW8), da(va, sizeof(int) * n), dc(vb, sizeof(int) * n);
    if (db.e || da.e || dc.e) return (int)(db.e ? db.e : da.e ? da.e : dc.e);
    hipLaunchKernelGGL(k_store_row8, dim3(n / 256), dim3(256), 0, 0, (uint8_t*)db.p, (const int*)da.p, (const int*)dc.p, s, mode);
    if (int e = finish()) return e;
    return (int)db.back(buf);
}

// One workgroup per problem: total = npad + guard keys of LDS, loaded from and written back to io[block][total]; the sort gets the
// first npad, the guard keys behind them must come back as they went in.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_bitonic(u64* io, int npad, int total) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);
    io += (size_t)blockIdx.x * total;
    for (int i = threadIdx.x; i < total; i += THREADS) keys[i] = io[i];
    __syncthreads();
    bitonic_sort_lds<THREADS>(keys, npad);
    for (int i = threadIdx.x; i < total; i += THREADS) io[i] = keys[i];
}
extern "C" int dh_bitonic(u64* io, int npad, int guard, int blocks, int threads) {
    const size_t lds = (size_t)(npad + guard) * sizeof(u64);
    if (npad < 64 || npad > VISO_SORT_MAX || (npad & (npad - 1)) || guard < 64 || lds > 160 * 1024 || blocks <= 0 ||
        (threads != 256 && threads != 512))
        return -1;   // (guard >= 64: a comparator loop that runs to a full wave of 64 reaches no index beyond npad + 63)
    Dev d(io, lds * blocks);
    if (d.e) return (int)d.e;
    const void* f = threads == 512 ? (const void*)k_bitonic<512> : (const void*)k_bitonic<256>;
    if (hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return (int)e;
    if (threads == 512) hipLaunchKernelGGL(k_bitonic<512>, dim3(blocks), dim3(512), lds, 0, (u64*)d.p, npad, npad + guard);
    else hipLaunchKernelGGL(k_bitonic<256>, dim3(blocks), dim3(256), lds, 0, (u64*)d.p, npad, npad + guard);
    if (int e = finish()) return e;
    return (int)d.back(io);
}

// ---- voxel_hash.h ---------------------------------------------------------------------------------------------------------------
DH_KERNEL(map_hash, u64, 1, NONE, NONE, uint32_t, 1, out[0] = map_hash(a[0]);)
// (kx, ky, kz), d -> the key, its neighbour at corner d, the key taken apart again
DH_KERNEL(voxel_key, int, 3, uint32_t, 1, NONE, long long, 5, const u64 k = voxel_key(a[0], a[1], a[2]); int32_t u[3]; voxel_unkey(k, u);
          out[0] = (long long)k; out[1] = (long long)voxel_neighbour(k, b[0]); out[2] = u[0]; out[3] = u[1]; out[4] = u[2];)
extern "C" void dh_host_voxel_key(const int* a, const uint32_t* d, long long* out, int n) {   // the same inline functions, compiled for the host
    for (int i = 0; i < n; ++i) {
        const u64 k = voxel_key(a[3 * i], a[3 * i + 1], a[3 * i + 2]);
        int32_t u[3];
        voxel_unkey(k, u);
        out[5 * i] = (long long)k; out[5 * i + 1] = (long long)voxel_neighbour(k, d[i]);
        out[5 * i + 2] = u[0]; out[5 * i + 3] = u[1]; out[5 * i + 4] = u[2];
    }
}
DH_KERNEL(voxel_runs, u64, 1, NONE, NONE, int, 3, bool head; uint32_t len; voxel_runs(a[0], lane, &head, &len);
          out[0] = head; out[1] = (int)len; out[2] = voxel_run_head(head, lane);)

__global__ __launch_bounds__(256) void k_list_position(VoxelTable t, const int* take, u64* at, int* ret) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    u64 pos = ~0ull;
    const bool tk = take[i] != 0;
    ret[i] = voxel_list_position(t, tk, threadIdx.x & 63, &pos);
    at[i] = pos;
}
extern "C" int dh_list_position(const int* take, u64* at, int* ret, u64* total, int n) {
    if (n <= 0 || n % 256) return -1;
    const u64 zeros[32] = {0};
    Dev dw(zeros, sizeof zeros), dt(take, sizeof(int) * n), da(at, sizeof(u64) * n), dr(ret, sizeof(int) * n);
    if (dw.e || dt.e || da.e || dr.e) return (int)(dw.e ? dw.e : dt.e ? dt.e : da.e ? da.e : dr.e);
    VoxelTable t{nullptr, nullptr, (u64*)dw.p, 0u};
    hipLaunchKernelGGL(k_list_position, dim3(n / 256), dim3(256), 0, 0, t, (const int*)dt.p, (u64*)da.p, (int*)dr.p);
    if (int e = finish()) return e;
    u64 w[32];
    if (hipError_t e = dw.back(w)) return (int)e;
    *total = w[VOXEL_W_OUT];
    if (hipError_t e = da.back(at)) return (int)e;
    return (int)dr.back(ret);
}

__global__ __launch_bounds__(256) void k_voxel_probe(u64* table, uint32_t mask, const u64* keys, uint32_t* slot, int* claimed, int* ret) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    uint32_t s = 0xffffffffu;
    bool cl = false;
    ret[i] = voxel_probe(table, mask, keys[i], &s, &cl);
    slot[i] = s; claimed[i] = cl;
}
__global__ __launch_bounds__(256) void k_voxel_find(const u64* table, uint32_t mask, const u64* keys, uint32_t* slot, int* ret) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    uint32_t s = 0xffffffffu;
    ret[i] = voxel_find(table, mask, keys[i], &s);
    slot[i] = s;
}
// table: `slots` keys (a power of two), in and out for the probe; claimed == null: voxel_find (reads only)
extern "C" int dh_voxel_probe(u64* table, int slots, const u64* keys, int n, uint32_t* slot, int* claimed, int* ret) {
    if (n <= 0 || n % 256 || slots < 2 || (slots & (slots - 1))) return -1;
    Dev dt(table, sizeof(u64) * slots), dk(keys, sizeof(u64) * n), ds(slot, sizeof(uint32_t) * n), dc(claimed, claimed ? sizeof(int) * n : 0),
        dr(ret, sizeof(int) * n);
    if (dt.e || dk.e || ds.e || dc.e || dr.e) return (int)(dt.e ? dt.e : dk.e ? dk.e : ds.e ? ds.e : dc.e ? dc.e : dr.e);
    if (claimed)
        hipLaunchKernelGGL(k_voxel_probe, dim3(n / 256), dim3(256), 0, 0, (u64*)dt.p, (uint32_t)slots - 1u, (const u64*)dk.p, (uint32_t*)ds.p,
                           (int*)dc.p, (int*)dr.p);
    else
        hipLaunchKernelGGL(k_voxel_find, dim3(n / 256), dim3(256), 0, 0, (const u64*)dt.p, (uint32_t)slots - 1u, (const u64*)dk.p,
                           (uint32_t*)ds.p, (int*)dr.p);
    if (int e = finish()) return e;
    if (claimed) {
        if (hipError_t e = dt.back(table)) return (int)e;
        if (hipError_t e = dc.back(claimed)) return (int)e;
    }
    if (hipError_t e = ds.back(slot)) return (int)e;
    return (int)dr.back(ret);
}

// ---- solver_dev.h ---------------------------------------------------------------------------------------------------------------
DH_KERNEL(lu_solve6, double, 36, double, 6, NONE, double, 7, double A[6][6]; double B[6];   // -> b[6] as lu_solve6 leaves it, the verdict
          for (int r = 0; r < 6; ++r) { B[r] = b[r]; for (int q = 0; q < 6; ++q) A[r][q] = a[r * 6 + q]; }
          const int ok = lu_solve6(A, B);
          for (int r = 0; r < 6; ++r) out[r] = B[r];
          out[6] = (double)ok;)
DH_KERNEL(sample3, u64, 3, int, 1, NONE, int, 3, int t[3]; viso_sample3(a[0], a[1], (int)a[2], b[0], t); out[0] = t[0]; out[1] = t[1]; out[2] = t[2];)
DH_KERNEL(splitmix64, u64, 1, NONE, NONE, u64, 2, u64 s = a[0]; out[0] = viso_splitmix64(&s); out[1] = s;)
DH_KERNEL(mulhi64, u64, 1, u64, 1, NONE, u64, 1, out[0] = viso_mulhi64(a[0], b[0]);)
DH_KERNEL(up6, int, 1, int, 1, NONE, int, 1, out[0] = up6(a[0], b[0]);)
extern "C" void dh_host_sample3(const u64* a, const int* N, int* out, int n) {   // the host compilation of the same inline functions
    for (int i = 0; i < n; ++i) viso_sample3(a[3 * i], a[3 * i + 1], (int)a[3 * i + 2], N[i], out + 3 * i);
}
extern "C" void dh_host_splitmix64(const u64* a, u64* out, int n) {
    for (int i = 0; i < n; ++i) { u64 s = a[i]; out[2 * i] = viso_splitmix64(&s); out[2 * i + 1] = s; }
}
extern "C" void dh_host_mulhi64(const u64* a, const u64* b, u64* out, int n) {
    for (int i = 0; i < n; ++i) out[i] = viso_mulhi64(a[i], b[i]);
}
// One workgroup per problem: Li [36], sigma2 -> cov [36]
__global__ __launch_bounds__(256) void k_write_cov6(const double* Li, const double* sigma2, double* cov) {
    write_cov6(Li + blockIdx.x * 36, sigma2[blockIdx.x], cov + blockIdx.x * 36);
}
extern "C" int dh_write_cov6(const double* Li, const double* sigma2, double* cov, int nb) {
    if (nb <= 0) return -1;
    Dev dl(Li, sizeof(double) * 36 * nb), ds(sigma2, sizeof(double) * nb), dc(cov, sizeof(double) * 36 * nb);
    if (dl.e || ds.e || dc.e) return (int)(dl.e ? dl.e : ds.e ? ds.e : dc.e);
    hipLaunchKernelGGL(k_write_cov6, dim3(nb), dim3(256), 0, 0, (const double*)dl.p, (const double*)ds.p, (double*)dc.p);
    if (int e = finish()) return e;
    return (int)dc.back(cov);
}
