// common.h — shared declarations of libviso_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <atomic>

#include "../../include/viso_hip.h"

#define VISO_ROW 128          // packed descriptor row: 128 x u16 = 256 B (121 used, rest = bias)
#define VISO_ROW8 128         // bytes of a row's 8-bit plane (ImageView::rows8)
// The planes' element is h_s(v) = clamp((v + (128 << s)) >> s, 0, 255) with a shift s in 0..3 chosen per RUN from the data:
// every 16th run of a batch (and its first) the pack kernels count, over a sample of rows, how many element pairs reach
// 128 / 256 / 512 (VISO_R8_*), the counts come back through a pinned buffer behind an event, and the host gives the runs
// after that the smallest s that clamps at most 1 pair in 256 — as a kernel argument.  (SAD8 << s) - VISO_ROW8_SLACK(s) <=
// SAD for ANY descriptors and any s: a wrong s costs time (more candidates scored exactly), never a result.
#define VISO_ROW8_SLACK(S) (((1 << (S)) - 1) * VISO_ROW8)   // at most 128 elements count, each off by at most 2^s - 1
#define VISO_R8_C128 0        // int cnt[4] per batch (8-byte aligned): [0..2] sampled element pairs (lanes of the pack kernels) whose
#define VISO_R8_ROWS 3        //   larger magnitude reaches 128 / 256 / 512, [3] sampled rows
#define VISO_R8_DEFAULT 3     // shift before any statistics exist (covers the whole range of a 3x3 Sobel of uint8)
#define VISO_R8_EVERY 16      // runs between two looks at the data
#define VISO_PACK_SUMS 1      // pack kernels, `extras`: also write ImageView::sums (matcher variant 5)
#define VISO_PACK_ROWS8 2     //                         also write ImageView::rows8 (matcher variant 6)
#define VISO_BIAS 32768       // u16 = int16 value + 32768 (SAD is translation invariant)
#define VISO_WAVE 64
#define VISO_QCAP 256         // per-wave candidate queue entries
#define VISO_QPB 32           // queries per workgroup in the matcher
#define VISO_MATCH_THREADS 256
#define VISO_KPCAP 768        // target-window keypoints staged in LDS per query tile
#define VISO_NB 256           // column buckets of the per-image x index
#define VISO_SORT_MAX 16384   // keypoints per image / queries per call (LDS bitonic sorts)

void viso_set_error(const char* fmt, ...);

#define HIP_TRY(expr)                                                              \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) {                                                    \
            viso_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr,           \
                           hipGetErrorString(_e));                                 \
            return VISO_ERR_HIP;                                                   \
        }                                                                          \
    } while (0)

// a call of this library's own: its error (the text is set) is the caller's
#define VISO_TRY(expr)                                                             \
    do {                                                                           \
        const int _r = (expr);                                                     \
        if (_r < 0) return _r;                                                     \
    } while (0)

// ---- device-side views -----------------------------------------------------
struct MatchParamsDev {          // viso_match_params, device copy (kernarg)
    int epi, second, K, _pad;
    float radius, _padf;
    double F[9];
    double sampson_thresh, ratio;
};

struct ImageView {               // one image's keypoints + descriptors on the device
    const float2* kp;            // [n] boundary order (x,y)
    const float* frows;          // [n][dlen] boundary-layout descriptors (original order)
    const int* n;                // keypoint count (device, ragged batches)
    float2* skp;                 // [n] keypoints grouped by column bucket (counting sort by bucket_of(x): 256 buckets over
                                 //     the image's x range).  NO order inside a bucket (scattered with LDS atomics), and
                                 //     keypoints with a NaN x share the last bucket with the largest columns.
    int* sidx;                   // [n] bucket-order position -> original index
    int* rank;                   // [n] original index -> bucket-order position
    int* bstart;                 // [VISO_NB+1] first sorted position of each column bucket
    float* xinfo;                // [8] x0, scale of the column bucket map; smallest and largest finite keypoint y;
                                 //     [4] number of keypoints whose x is not NaN, as a float: a COUNT only, not a prefix
                                 //     length (NaN-x keypoints sit anywhere inside the last bucket)
    uint8_t* qord;               // [n rounded up to 64] y order inside every block of 64 bucket-order positions: entry B*64 + r =
                                 //     offset (0..63) in block B of the keypoint with y rank r (positions past n rank last)
    uint16_t* rows;              // [n][128] packed descriptor rows, bucket order
    uint2* sums;                 // [n] bucket order: sums of the row's four 32-element blocks, each clamped to int16 and
                                 //     biased like the elements (4 x u16).  sum_k |S_q,k - S_t,k| <= SAD(q, t) (triangle
                                 //     inequality per block; clamping is 1-Lipschitz): the lower bound match_prune_kernel
                                 //     prunes candidates with.  Written by the pack kernels together with the rows.
    uint8_t* rows8;              // [n][128] bucket order: the rows' 8-bit plane, element h_s(v) = clamp((v + (128 << s)) >> s, 0, 255)
                                 //     (pad = h_s(0)), s = the run's shift (a kernel argument, see VISO_R8_*).  2^s |h(a) - h(b)| - (2^s - 1) <= |a - b|
                                 //     for ANY a, b (floor and clamp are monotone and 1-Lipschitz in units of 2^s), so
                                 //     (SAD8 << s) - VISO_ROW8_SLACK(s) <= SAD: the lower bound match_union8_kernel ranks candidates
                                 //     with.  Written by the pack kernels when matcher variant 6 is selected.
    int* bad;                    // [1] != 0: this image's descriptors do not fit the u16 rows (pack_desc_kernel);
                                 //     every problem that reads the image then takes the general (double) kernel
};

struct MatchProblem {            // one match_desc call (reference src/viso.cpp:669)
    ImageView q, t;              // queries (kp1,d1) and targets (kp2,d2)
    int2* res;                   // per ORIGINAL query index: (accepted target or -1, (int)best SAD)
    int* sorted;                 // out: M x 3 (i1,i2,dist) sorted by (dist,i1)
    int* pos;                    // out: per query, row in `sorted` or -1
    int* m_cnt;                  // out: M
    unsigned long long* scored;  // out: number of SAD evaluations (C of SURVEY 8(d))
    int2* ovf;                   // scratch shared by ALL problems of a launch: (problem, sorted position) of every query
    int* ovf_cnt;                //     left to the overflow kernel, and their count (zeroed before every run) — one
                                 //     queue, so that the overflow kernel's waves share the work evenly whatever
                                 //     problem it comes from (dense keypoint clusters concentrate it in a few problems)
    int* tile_flag;              // scratch, stereo call: per 64-query tile, 1 = match_batch_kernel<1> does the tile
                                 //     (written by match_stereo_kernel for every tile, read by the kernel behind it)
    int pidx;                    // 0 = stereo params, 1 = temporal params
    int cap;                     // row capacity of res/sorted/pos
};

struct SolverParamsDev {         // viso_param, device copy
    double base, f, cu, cv, inlier_threshold, thresh;
    int ransac_iter, _pad;
};

// The scratch blocks of a context (ctx_scratch).  The DEFAULT context's are shared by the plain family and the direct calls; a direct
// call that names a context (the loop-closure calls, DirectCall::begin(ctx)) uses that context's own blocks.  Every user holds
// PlainLock and issues ALL its work on the context's stream, and a block is regrown only behind a synchronize of that stream: a
// slot's users are ordered by the stream -- behind a frame's RANSAC stage that runs on after its call returned, too -- so a call may
// use any slot for contents that need not outlive it.  zero_new promises zeros at (re)allocation and nothing more: its user hands
// the block back zeroed and relies on finding it so, which is why SLOT_RANSAC_QUEUE must not be borrowed.
enum ScratchSlot {
    SLOT_GEN0 = 0, SLOT_GEN1, SLOT_GEN2,   // general: a direct call's staged inputs and outputs, any element type
    SLOT_HARRIS_TMP_RESP,                  // viso_detect_harris_binned: the bins' candidate responses
    SLOT_HYP_WORDS,                        // per-hypothesis ints (ok_h, cnt_h) of the RANSAC chain and viso_support_sizes; the bins' counters
    SLOT_HYP_TR,                           // the hypotheses' transforms tr_h; viso_detect_harris_binned: the kept keypoints
    SLOT_GEN6,                             // viso_detect_harris_binned: the kept responses; viso_support_sizes: its SolverItem
    SLOT_HARRIS_STRIPS,                    // viso_detect_harris_binned: the strip kernel's partial lists
    SLOT_RANSAC_QUEUE,                     // zero_new: the undecided-hypothesis queue, left zeroed by every chain (launch_ransac)
    SLOT_RANSAC_ROT,                       // the hypotheses' rotation block (SolverItem::rot)
    SLOT_UNUSED10, SLOT_UNUSED11, SLOT_UNUSED12, SLOT_UNUSED13,   // no user (kept: the numbering of the others stays)
    SLOT_PLAIN_IN, SLOT_PLAIN_OUT,         // PlainStage's device mirror; a plain-family call's result block
    SLOT_CIRCLE_TAB,                       // the circle / RANSAC-stage join table (launch_circle_table)
    SLOT_SUBPIX_IMG, SLOT_SUBPIX_KP, SLOT_SUBPIX_LIST, SLOT_SUBPIX_UV,   // viso_refine_stereo_subpixel
    SLOT_RECT_RAW, SLOT_RECT_OUT, SLOT_RECT_MAP,                          // viso_rectify_images
    SLOT_COUNT
};

struct viso_ctx {
    int device;
    hipStream_t stream;
    bool own_stream;
    int matcher_variant;         // viso_ctx_set_matcher
    int row8_force;              // viso_ctx_set_row8_shift: -1 = chosen from the data (default), 0..3 = fixed
    int gn_split;                // viso_ctx_set_gn_split
    // second stream of the context: the RANSAC stage of its batches runs here, beside the next run's
    // matcher on `stream` (viso_ctx_synchronize waits for both).  One per CONTEXT, not per batch: the runtime maps
    // streams onto a handful of hardware queues, and two busy RANSAC streams that land on one queue serialise
    // (measured: 9 streams for 3 busy batches -> two chains on one queue, 0.43 -> 0.68 ms per step).
    hipStream_t solver_stream;
    // grow-only scratch for the plain (host-pointer) family, one block per ScratchSlot
    void* scratch[SLOT_COUNT];
    size_t scratch_bytes[SLOT_COUNT];
    // pinned staging of the plain family (grow-only): [0] a call's inputs, packed back to back and sent with ONE
    // host-to-device copy; [1] a call's results, fetched with ONE device-to-host copy behind ONE synchronize
    char* pin[2];
    size_t pin_bytes[2];
    struct PlainCache* plain;    // the plain family's image cache (plain.hip), created on first use
    // completion signal of the plain family's calls (PlainSignal below): a word of pinned memory the call's LAST kernel writes,
    // a device counter of that kernel's finished workgroups, the sequence number of the last signal asked for
    int* sig_flag; int* sig_ctr; uint32_t sig_seq;   // the number wraps; the wait compares differences
    unsigned long long serial;   // unique per created context: a voxel map tells its own context from a later one at the same address
};

// handle registry (ctx.hip): the live contexts, the live batches of each, tombstones of batches their context took along
struct viso_batch;
bool viso_ctx_live(const viso_ctx* c);
bool viso_batch_live(const viso_batch* b);
bool viso_batch_register(viso_ctx* c, viso_batch* b);   // false: the context is not live
int viso_batch_unregister(viso_batch* b);               // 1 live (now the caller's to free), 0 tombstone (consumed), -1 unknown
int viso_batch_free(viso_batch* b, bool keep_shell);    // batch.hip: frees a batch that has left the registry (keep_shell: the host object stays for the caller's late destroy)

struct PlainLock { PlainLock(); ~PlainLock(); };   // serialises the plain family on the default context
// viso_plain_profile: phases of one plain-family call, bracketed by four events on the call's stream (ctx.hip).  Used
// inside a PlainLock.  mark(1) = inputs enqueued, mark(2) = kernels enqueued, mark(3) = results on the host.
struct PlainProf {
    void start(int fn, hipStream_t s);   // records event 0
    void close();                        // adds the call to its function's times; once
    ~PlainProf() { close(); }
    void mark(int k);
    void wait_begin();
    void wait_end();
    int fn = 0; hipStream_t s = nullptr; bool on = false; int marks = 0; double t0 = 0, tw = 0, wait = 0;
};
int ctx_scratch(viso_ctx* c, ScratchSlot slot, size_t bytes, void** out, bool zero_new = false);   // zero_new: a block that is (re)allocated starts zeroed
static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }   // offsets of the pieces of a scratch block
int ctx_pinned(viso_ctx* c, int which, size_t bytes, char** out);
void plain_cache_free(viso_ctx* c);   // plain.hip; from viso_ctx_destroy
// plain.hip: a call of the reference's loop that the frame's stereo call has already answered (1 = served, 0 = go to the device)
int plain_try_collect(viso_ctx* c, const float* kp1, int n1, const float* kp2, int n2, const int32_t* match, int n, double* x);
int plain_try_triangulate(viso_ctx* c, const double* x, int m, const viso_param* p, double* X);
int plain_try_circle(viso_ctx* c, const int32_t* lr, int n_lr, const int32_t* lr_prev, int n_lrp, const int32_t* m11, int n11,
                     const int32_t* m22, int n22, int32_t* circ, int32_t* pcl, int cap, int* out_n, int* ret);
void plain_note_circle(viso_ctx* c, int cnt);
int plain_try_ransac(viso_ctx* c, const double* X, const double* obs, int m, double best_tr[6], int32_t* best_inl, int* n_inl,
                     const viso_param* p, const int32_t* samples, uint64_t seed, uint64_t frame, int* ret);

struct PlainSignal { int* ctr; int* flag; uint32_t seq; };   // a call's completion signal (described below); flag == nullptr: no signal
struct OutArgs;                                          // a copy-out into the call's pinned mirror (below)
// match_circle on lists in device memory (circle.hip): counts by value, or read from the device when the pointers are set
struct CircleArgs {
    const int* lr; const int* lrp; const int* m11; const int* m22;
    int n_lr, n_lrp, n11, n22;
    const int* n_lr_p; const int* n_lrp_p; const int* n11_p; const int* n22_p;   // device counts (override the values), or null
    int* rows;      // out: 6 ints per joined row: circ_match (ileft, iright, ileft_prev, iright_prev) | match_pcl (i, k)
    int cap; int* out_n;
    // optional (the plain family's frames; g_x == null: no gather): x_c / Xp_c of src/viso.cpp:1292-1305 -- columns of this frame's x
    // and of the previous frame's X picked by match_pcl -- written by the kernel's tail instead of a kernel of their own
    const double* g_x; const double* g_Xp; double* g_xc; double* g_Xpc; int g_ldx, g_ldXp, g_ldc;
    // optional (plain family): a copy-out of the kernel BEFORE this one rides in the launch as ride_blocks extra workgroups
    // (OutArgs in device memory; plain_out_blocks)
    const OutArgs* ride; int ride_blocks;
};
// tab: 3 * tabn ints of device scratch; keys outside [0, tabn) or duplicate keys take the literal nested loops
int launch_circle_table(hipStream_t s, const CircleArgs& a, int* tab, int tabn);
viso_ctx* viso_default_ctx();
// "The caller passed ctx_or_null": a handle that is not live is VISO_ERR_ARG, "<where>: not a live context handle" (where == null: the
// text without the prefix); null is the default context (none: VISO_ERR_HIP, viso_ctx_create's message stays).  out == null: the
// check alone, which touches no device.
int ctx_resolve(const char* where, viso_ctx* ctx_or_null, viso_ctx** out);

// One direct call: a batch stage's kernel on host pointers, on the default context or on one the caller names (ctx.hip).  Declared behind the argument checks
// and the early VISO_OK returns, which touch no device.  An error return must not leave work in flight (plain_quiesce, plain.hip):
// copies into or out of the caller's memory may be queued on s, and the scratch blocks they use are the next caller's.  So the
// destructor waits for s, before it gives the lock back, unless the last thing the call did was a wait() that succeeded.
// PlainCall (below) is its sibling for the plain family's small signalled calls, under the same rule.
struct __attribute__((visibility("hidden"))) DirectCall {
    viso_ctx* c = nullptr; hipStream_t s = nullptr;
    DirectCall() = default;
    DirectCall(const DirectCall&) = delete;
    ~DirectCall();
    // PlainLock's mutex, then the context -- ctx (live: the caller has checked), its device, stream and scratch blocks, or with null the
    // default context (none: VISO_ERR_HIP, viso_ctx_create's message stays) -- and hipSetDevice
    int begin(viso_ctx* ctx = nullptr);
    template <class T> int scratch(ScratchSlot slot, size_t count, T** out, bool zero_new = false) { return ctx_scratch(c, slot, sizeof(T) * count, (void**)out, zero_new); }
    // count elements of the HOST pointer's type, on s; count 0 copies nothing
    template <class T> int up(void* dst_dev, const T* src_host, size_t count) { return copy(dst_dev, src_host, sizeof(T) * count, hipMemcpyHostToDevice); }
    template <class T> int down(T* dst_host, const void* src_dev, size_t count) { return copy(dst_host, src_dev, sizeof(T) * count, hipMemcpyDeviceToHost); }
    int wait();    // hipStreamSynchronize(s): the results are in the caller's memory
private:
    int copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind);
    bool locked = false, in_flight = false;
};

// One plain-family call's inputs: appended to the context's pinned block (256-B aligned pieces), mirrored at the same
// offsets in one device block, sent with ONE hipMemcpyAsync.  A pageable hipMemcpyAsync costs 5-10 us of host time
// per call whatever its size; the plain family used to issue 4-7 of them per function (tools/h2d_probe.hip).
struct PlainStage {
    char* h = nullptr; char* d = nullptr; size_t off = 0, cap = 0;
    static size_t need(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    int begin(viso_ctx* c, size_t bytes) {
        cap = bytes; off = 0;
        int r = ctx_pinned(c, 0, bytes, &h);
        if (r < 0) return r;
        return ctx_scratch(c, SLOT_PLAIN_IN, bytes, (void**)&d);
    }
    template <class T> T* put(const T* src, size_t count) {   // returns the DEVICE address
        const size_t b = sizeof(T) * count;
        if (b) __builtin_memcpy(h + off, src, b);
        T* r = reinterpret_cast<T*>(d + off);
        off += need(b);
        return r;
    }
    template <class T> T* host_of(const T* dev) const { return reinterpret_cast<T*>(h + (reinterpret_cast<const char*>(dev) - d)); }
    // Small blocks go through a copy KERNEL that reads the pinned block over PCIe itself: the copy engine costs ~10 us
    // of latency per transfer whatever its size, a launch 2-3 (tools/h2d_probe.hip: H2D + kernel + D2H + synchronize
    // 29 us by copy engine, 18 us by copy kernels).
    int flush(hipStream_t s);
};
// words = 32-bit units.  dst[0..head) = src[0..head), then min(*n_rows, max_rows) rows of row_words behind them (n_rows
// may be null: head only).  Either side may be pinned host memory.
// A plain-family call returns when its results are in pinned host memory.  hipStreamSynchronize sees that ~5 us after the
// fact (an empty kernel + synchronize: 10.9 us; the same kernel writing a word of pinned memory that the host spins on:
// 6.2 us -- tools/h2d_probe.hip).  So the call's LAST kernel -- a copy kernel into pinned memory -- signals itself: every thread
// fences its stores at system scope, the last workgroup to finish (a device counter) release-stores the call's sequence
// number into a pinned word, and the host spins on that word with an acquire load (plain_signal_wait: bounded, then
// hipStreamSynchronize as the fallback, so a lost signal costs time, never a hang or a result).
int plain_signal_next(viso_ctx* c, PlainSignal* out);   // the next sequence number of the context (allocates on first use)
int plain_signal_wait(viso_ctx* c, hipStream_t s, uint32_t seq);
int plain_blit(hipStream_t s, const void* src, void* dst, size_t head_words, const int* n_rows = nullptr, int row_words = 0, int max_rows = 0,
               const PlainSignal* sig = nullptr);
// One small signalled call of the plain family on the default context (ctx.hip), DirectCall's sibling: declared behind the argument
// checks and the early returns that touch no device.  The steps of every such call, in this order:
//   begin(fn); inputs() / in.put; result(); sent(); the launch; launched(); signal() or fetch(); wait(); read the mirror; done().
// The same rule holds: an error return must not leave work in flight -- the copy kernel of sent() reads the context's pinned block
// over PCIe, and the next call overwrites that block.  So the destructor waits for s, before the lock goes back, when something of
// this call may be queued (a flush, a launch, a signal asked for) and the last thing the call did was not a wait() that succeeded.
// The returns with nothing queued (a plain_try_* answer, an allocation that failed before sent()) and the success path wait for nothing.
struct __attribute__((visibility("hidden"))) PlainCall {
    viso_ctx* c = nullptr; hipStream_t s = nullptr;
    PlainProf pp;                         // viso_plain_profile's times of this call
    PlainStage in;                        // the inputs: inputs(bytes), then in.put, in.host_of
    char *dout = nullptr, *hout = nullptr;   // result(): the device block (on_device) and its pinned mirror
    PlainCall() = default;
    PlainCall(const PlainCall&) = delete;
    ~PlainCall();
    // PlainLock's mutex, the default context (none: VISO_ERR_HIP, viso_ctx_create's message stays), hipSetDevice, the profile's start
    int begin(int fn);
    int inputs(size_t bytes) { return in.begin(c, bytes); }
    int result(size_t bytes, bool on_device);   // hout = the pinned mirror, dout = SLOT_PLAIN_OUT when asked for
    int sent(bool flush = true);          // the inputs are on their way (flush = false: the kernel reads the pinned block itself); mark(1)
    void launched() { queued = true; pp.mark(2); }
    int signal(PlainSignal* out);         // the call's signal, for a last kernel that signals itself
    // ... or a copy kernel of dout's first head_words words and the n_rows rows that exist into hout (plain_blit), which signals
    int fetch(size_t head_words, const int* n_rows = nullptr, int row_words = 0, int max_rows = 0);
    int wait();                           // the signal has come: the results are in hout
    void done() { pp.mark(3); }
private:
    uint32_t seq = 0; bool locked = false, queued = false;
};
#ifdef __HIPCC__
// Called by EVERY thread of the kernel's every workgroup, behind its last store.
__device__ __forceinline__ void plain_signal_done(const PlainSignal& g, unsigned nblocks) {
    if (!g.flag) return;                       // uniform
    __threadfence_system();                    // this thread's stores (to pinned host memory) are out, system scope
    __syncthreads();
    if (threadIdx.x == 0) {
        if (atomicAdd(g.ctr, 1) == (int)nblocks - 1) {   // the last workgroup of the launch: every other one has fenced and counted
            __threadfence_system();                      // (acquire side of the counter: what the others fenced is ordered before the flag)
            *g.ctr = 0;                                  // for the next signalling kernel (streams run them one after the other)
            __hip_atomic_store(g.flag, (int)g.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
#endif
// ---- results out: every region's rows that exist (counts on the device) into the call's pinned mirror ----------------------
// A workgroup's path to host memory is narrow (a single one needs 15 us for what 39 spread over the chip write in 4), so the
// copy is many small workgroups -- and where the chain has a next kernel they RIDE in its launch as extra workgroups (the
// copy-out of the sort kernel's lists in the join kernel's launch, the join's in ransac_coop_kernel's): they depend on the
// kernel before, not on the one they ride in, and the 8.5 us + launch gap of a copy kernel of their own leave the chain.
// The last kernel of the chain, ransac_refit_kernel, writes its few hundred bytes itself (RefitMirror).
struct OutRegion { const uint32_t* src; uint32_t* dst; const int* cnt; int row_words, max_rows; };
#define OUT_REGIONS 16
struct OutArgs { OutRegion r[OUT_REGIONS]; int n_regions, gx; PlainSignal sig; };   // gx workgroups of 256 threads' worth per region
#ifdef __HIPCC__
// workgroup `b` of n_regions * gx (any workgroup size; every thread calls)
__device__ __forceinline__ void plain_out_blocks(const OutArgs& a, unsigned b) {
    const OutRegion R = a.r[b / (unsigned)a.gx];
    const unsigned bx = b % (unsigned)a.gx;
    int n = R.max_rows;
    if (R.cnt) { const int c = *R.cnt; n = c < 0 ? 0 : c < n ? c : n; }
    const unsigned total = (unsigned)n * (unsigned)R.row_words;
    for (unsigned i = bx * blockDim.x + threadIdx.x; i < total; i += (unsigned)a.gx * blockDim.x) R.dst[i] = R.src[i];
    plain_signal_done(a.sig, (unsigned)(a.n_regions * a.gx));
}
#endif
struct RefitMirror {                 // ransac_refit_kernel, n_items == 1: the result block and the inliers that exist, copied by the workgroup, which signals
    const uint32_t* res_src; uint32_t* res_dst; int res_words;
    const int* n_inl; const uint32_t* inl_src; uint32_t* inl_dst; int max_inl;
    PlainSignal sig;
};

// ---- launchers (host) -------------------------------------------------------
// group every image's keypoints by column bucket (+ inverse permutation, column index, y order inside 64-blocks)
// zero_words / n_zero: optional 32-bit words the kernel zeroes on the way (a run's counters: one memset less in front of it)
// r8zero: the batch's four VISO_R8_* counters, zeroed too when the run is one that counts (or null)
// imp (plain family, n_img == n_imp <= 2, imgs_dev unused): the images come from pinned HOST memory -- an image's view rides in the kernel arguments, the
// kernel reads the keypoints over PCIe, leaves them in view.kp, writes *view.n = n, *view.bad = bad0 and a copy of the view
// at view_dst (where the pack kernel's launch finds it): the copy kernel that used to run in front is gone
struct KpImport { const float2* src_kp; int n, bad0; ImageView* view_dst; ImageView view; };
int launch_sort_kp(hipStream_t s, const ImageView* imgs_dev, int n_img, int cap_max, uint32_t* zero_words = nullptr, int n_zero = 0,
                   int* r8zero = nullptr, const KpImport* imp = nullptr, int n_imp = 0);
// pack boundary-layout float descriptors into biased u16 rows in bucket order;
// sets the image's own flag (ImageView::bad) and *bad_any when a value is not an integer in [-32768, 32767];
// dlen > 128 (rows do not fit) flags every image.  bad_img: the n_img flags, contiguous (for that case).
// extras: VISO_PACK_SUMS / VISO_PACK_ROWS8 — what the selected matcher variant reads beside the u16 rows (pack_extras)
int launch_pack(hipStream_t s, const ImageView* imgs_dev, int n_img, int cap, int dlen, int* bad_img, int* bad_any, int extras, int r8s, int* r8cnt);
// match_union8_kernel keeps a cell's SAD8 >> 7 in a byte whose value 255 marks "scored exactly": 127 elements x 255 = 32385
// stays below that, 128 x 255 does not.  Descriptors of 128 elements (the reference's have 121) take match_union_kernel
static inline int matcher_effective(int variant, int dlen) { return (variant == 6 && dlen > 127) ? 3 : variant; }
static inline int pack_extras(int variant, int dlen) { variant = matcher_effective(variant, dlen); return variant == 5 ? VISO_PACK_SUMS : variant == 6 ? VISO_PACK_ROWS8 : 0; }
// the same from int16 descriptors [n_img][cap][dlen] (viso_batch_upload_i16*): never flags anything
int launch_pack_i16(hipStream_t s, const ImageView* imgs_dev, int n_img, int cap, int dlen, const int16_t* desc16, int extras, int r8s, int* r8cnt);
// kinds: which problems the launch can contain (the plain family knows: one call = one problem) -- kernels that would
// find nothing to do are not launched.  VISO_KIND_TEMPORAL: problems without the epipolar gate, VISO_KIND_STEREO: with it.
#define VISO_KIND_TEMPORAL 1
#define VISO_KIND_STEREO 2
#define VISO_KIND_ALL 3
#define VISO_KIND_NO_WIDE 4      // (plain family) leave match_batch_kernel<1> out: the launcher expects no tile with a wide epipolar band --
                                 // the count of declined tiles comes back with the results, and the call is repeated if there was one
// bad: int[2] zeroed before the run ([0] any image flagged by the pack kernel, [1] scratch counter of the stereo kernels)
// general_possible = 0: the rows cannot be flagged (descriptors extracted on the device from uint8 images), the
// kernels of the general (double) path are not even launched
int launch_match(hipStream_t s, const MatchProblem* probs_dev, int n_probs, int cap_max, int dlen,
                 const MatchParamsDev mp[2], int* bad, hipEvent_t e0, hipEvent_t e1, int layout, int variant,
                 const int2* ovf_q, const int* ovf_cnt, int r8s, int general_possible = 1, int kinds = VISO_KIND_ALL);
const char* matcher_kernel_name(int variant);
#define VISO_MATCHER_DEFAULT 6
struct TriItem;
// tri / tri_sp (plain family, or null): collect_matches + triangulate_rectified of problem 0's list inside the sort kernel
int launch_sort(hipStream_t s, const MatchProblem* probs_dev, int n_probs, int cap_max, int flagged_empty = 0,
                const TriItem* tri = nullptr, const SolverParamsDev* tri_sp = nullptr);
void fill_match_params(MatchParamsDev* d, const viso_match_params* h);
void fill_solver_params(SolverParamsDev* d, const viso_param* h);


// ---- solver / circle / triangulation items (device-resident descriptors) ---
struct SolverItem {            // one ransac_minimize_reproj problem (one frame)
    const double* X;           // 3 x ld  previous-frame 3-D points
    const double* obs;         // 4 x ld  observations (uL,vL,uR,vR)
    const int* m_ptr;          // number of points (device)
    int ld;
    int _pad;
    const int* samples;        // iters x 3, or NULL -> splitmix64 stream
    int* samp_h;               // iters x 3   the triples in use (ransac_hyp_kernel: drawn, or copied from `samples`)
    unsigned long long frame;  // stream key
    double* tr_h;              // iters x 6   hypothesis transforms
    int* ok_h;                 // iters
    int* cnt_h;                // iters
    char* rot;                 // viso_rot_bytes(iters): the hypotheses' rotations for the counting kernel (ransac_rot_kernel)
    double* tr;                // 6  in/out (best_tr)
    int* ok;                   // 1
    int* n_inl;                // 1
    int* inl;                  // up to m
    int* kept;                 // null, or 1 word: set to 1 when the stage leaves best_tr as the caller passed it -- no hypothesis found any
                               //     support (best_tr is assigned only on improvement, src/viso.cpp:1564-1568) or m < 3 -- and `tr` is then
                               //     NOT written; 0 otherwise.  Null (the batch family: sequence_odometry passes zeros, :1312): `tr` gets zeros.
};

struct JoinItem {
    const int* lr; const int* lr_cnt;        // sorted stereo matches of frame t
    const int2* res11;                       // temporal-left results, per query
    const int2* res22;                       // temporal-right results, per query
    const int* pos_lrp; const int2* res_lrp; // previous frame's stereo: row of query / result
    const float2* kp1; const float2* kp2;    // keypoints of frame t (left, right): x_c is collect_matches of the joined rows
    const float2* kp1p; const float2* kp2p;  // keypoints of frame t-1: Xp_c is triangulate_rectified of the joined rows,
                                             // computed in the join itself (src/viso.cpp:501-514, 1137-1162, 1292-1305)
    int* circ; int* pcl; int* mc;            // outputs
    double* x_c; double* Xp_c; int ldc;      // 4 x ldc, 3 x ldc
    const float2* uv; const float2* uvp;     // refined right-image points of frame t / t-1 per stereo row (viso_batch_set_subpixel;
                                             // read by circle_join_subpixel_kernel only)
};

struct TriItem {
    const float2* kp1; const float2* kp2;
    const int* match; const int* m_cnt;   // n x 3 (i1,i2,dist)
    double* x; double* X; int ld;         // 4 x ld, 3 x ld (X may be NULL)
};

// queue: device scratch of 2 + n_items * iters ints (list of the hypotheses stage 1 leaves undecided); queue[0] must be ZERO
// when the chain starts: zero it at allocation -- every chain leaves it zero behind its reader (ransac_rot_kernel)
// split: iterations the lane-per-hypothesis kernel runs before it hands undecided hypotheses to the wave-per-hypothesis
// kernel (viso_ctx::gn_split; 100 = the lane kernel does everything)
int launch_ransac(hipStream_t s, const SolverItem* items_dev, int n_items, int iters,
                  unsigned long long seed, const SolverParamsDev& sp, int* queue, int split, int max_points,
                  const RefitMirror* mir = nullptr, const OutArgs* ride = nullptr, int ride_blocks = 0);
size_t viso_rot_bytes(int iters);   // bytes of SolverItem::rot
int launch_circle_join(hipStream_t s, const JoinItem* items_dev, int n_items, const SolverParamsDev& sp, bool subpixel = false);
int launch_collect_triangulate(hipStream_t s, const TriItem* items_dev, int n_items,
                               const SolverParamsDev& sp, int cap);
struct BatchMatchArgs {          // kernarg of match_batch_kernel / match_union_kernel (tiles of 64 queries)
    const MatchProblem* probs;
    int n_probs, bpp, gs, gf, gc;
    int vblocks;                 // match_batch_kernel: (problem, tile) slots the grid walks (the stereo instantiation gets a small grid)
    int* bad;                    // [0] "some image of this run is flagged": lets the (normally idle) general kernels leave at once
                                 // [1] tiles match_stereo_kernel left to match_batch_kernel<1> (0: that kernel leaves at once)
    int r8s, _pad8;              // the shift of the 8-bit planes this run (match_union8_kernel)
    MatchParamsDev mp[2];
};
int launch_match_batch(hipStream_t s, const MatchProblem* probs_dev, int n_probs, int cap_max,
                       const MatchParamsDev mp[2], int* bad, int layout, hipEvent_t e_mid, int variant, int r8s,
                       int kinds = VISO_KIND_ALL);
int launch_match_union_temporal(hipStream_t s, const BatchMatchArgs& a, long long blocks);
int launch_match_prune_temporal(hipStream_t s, const BatchMatchArgs& a, long long blocks);
int launch_match_union8_temporal(hipStream_t s, const BatchMatchArgs& a, long long blocks);
int launch_match_strip_temporal(hipStream_t s, const BatchMatchArgs& a64, int cap_max);
int launch_match_stereo(hipStream_t s, const BatchMatchArgs& a64, int cap_max);
// match_frame.hip: the stereo and the temporal problems of a handful of problems (one frame) in ONE launch
int launch_match_frame(hipStream_t s, const BatchMatchArgs& at, const BatchMatchArgs& as64, long long blocks_t, int cap_max);
#define VISO_FRAME_MAX_BLOCKS 256   // temporal grids up to this size (8 problem slots of 2000 keypoints) take the one-launch kernel
struct StereoImages {   // "these resident image pairs", for every launcher that reads them; only launch_rectify's `out` is written
    uint8_t* img; size_t fs, ss; int rows, cols, n;   // image (k, side) of frames 0 .. n-1 at img + k * fs + side * ss; ss == 0: one camera
    size_t px() const { return (size_t)rows * cols; }
};
// Frames f0 .. f0+n-1 of a block [..][sides][rows][cols] (sides 1: one camera's images): the one place that knows where they lie
inline StereoImages image_block(uint8_t* block, int rows, int cols, int f0, int n, int sides = 2) {
    const size_t px = (size_t)rows * cols;
    return StereoImages{block + (size_t)f0 * sides * px, sides * px, sides == 2 ? px : 0, rows, cols, n};
}
// subpixel.hip: the opt-in sub-pixel refinement of frames' stereo lists (viso_batch_set_subpixel); uv [im.n][cap]
struct SubpixLists { const float2* kp; size_t kp_stride; int cap; const int* lists; size_t list_stride; const int* m_cnt; };   // as SubpixArgs
struct SubpixLeftRows { const uint16_t* lrows; size_t lrows_stride; const int* lrank; size_t lrank_stride; };   // absent: W_L from the image
int launch_subpixel(hipStream_t s, const StereoImages& im, const SubpixLists& l, int mode, float2* uv, const SubpixLeftRows& left = {});
// rectify.hip: the opt-in rectification of raw images (viso_batch_set_rectify).  One entry per output pixel, quantised on the host:
// off = byte offset of tap (0,0) in the raw image; meta = fx | fy << 5 | inside bits of taps (0,0) (1,0) (0,1) (1,1) << 10..13
struct RectEntry { int off; unsigned meta; };
void rect_quantise(const float* mapx, const float* mapy, size_t n, int raw_rows, int raw_cols, RectEntry* out);
bool rect_geometry_ok(int raw_rows, int raw_cols, int out_rows, int out_cols);
// raw -> out, the frames and sides of out; map [sides][out.px()]
int launch_rectify(hipStream_t s, const StereoImages& raw, const StereoImages& out, const RectEntry* map, int border);
// disparity.hip: the opt-in dense disparity (viso_batch_set_disparity); frame f's map at out + f * ofs
bool disparity_params_ok(const viso_disparity_params* p);
bool disparity_geometry_ok(int rows, int cols);   // cols within what the kernel handles
int launch_disparity(hipStream_t s, const StereoImages& im, const viso_disparity_params* p, int16_t* out, size_t ofs);
// The cap on a dense feature's workspace (sgm.hip, speckle.hip): the frames go through it in groups of as many as fit under the cap
struct __attribute__((visibility("hidden"))) WorkspaceCap {
    std::atomic<size_t> cap; size_t dflt; const char *what, *setter;   // what, setter: for the message
    void set(size_t bytes) { cap.store(bytes ? bytes : dflt); }         // 0: back to the default
    // *group (or null) = how many of n_frames frames of frame_bytes each fit, at most max_group; not even one: VISO_ERR_NOMEM
    int frames(const char* where, int rows, int cols, size_t frame_bytes, int n_frames, size_t max_group, int* group) {
        size_t g = cap.load() / frame_bytes;
        if (g < 1) {
            viso_set_error("%s: one %d x %d frame needs %zu bytes of %s workspace, more than the cap (%s)", where, rows, cols, frame_bytes, what, setter);
            return VISO_ERR_NOMEM;
        }
        if (g > max_group) g = max_group;
        if (group) *group = (int)(g < (size_t)n_frames ? g : (size_t)n_frames);
        return VISO_OK;
    }
};
// sgm.hip: the opt-in semi-global matching (viso_batch_set_sgm); the maps addressed as in launch_disparity.  The frames go
// through the workspace ws in groups of `group` (>= 1) frames: ws holds group * sgm_frame_bytes.  sgm_group_frames: *group (or null)
// = how many of n_frames frames fit the workspace cap; not even one: VISO_ERR_NOMEM, the error text names `where`
bool sgm_params_ok(const viso_sgm_params* p);
size_t sgm_frame_bytes(int rows, int cols, int D);
int sgm_group_frames(const char* where, int rows, int cols, int D, int n_frames, int* group);
int launch_sgm(hipStream_t s, const StereoImages& im, const viso_sgm_params* p, int16_t* out, size_t ofs, void* ws, int group);
// speckle.hip: the opt-in speckle filter of the maps (viso_batch_set_speckle), in place; frame f's map at map + f * mfs.  The frames
// go through the workspace ws in groups of `group` (>= 1) frames: ws holds group * speckle_frame_bytes.  speckle_group_frames: as
// sgm_group_frames.
bool speckle_params_ok(const viso_speckle_params* p);
bool speckle_geometry_ok(int rows, int cols);   // cols as the methods, and rows * cols within the 32-bit labels
size_t speckle_frame_bytes(int rows, int cols);
int speckle_group_frames(const char* where, int rows, int cols, int n_frames, int* group);
int launch_speckle(hipStream_t s, int16_t* map, size_t mfs, int rows, int cols, int n_frames, const viso_speckle_params* p, void* ws,
                   int group);
// ---- "these disparity maps": what every consumer of the maps receives (the reprojection, the fuses, the alignments) ------------------
struct StereoCalib { double f, cu, cv, base; };
struct DispView {
    const int16_t* disp; size_t mfs;    // frame k's map at disp + k * mfs
    const uint8_t* image; size_t ifs;   // frame k's 8-bit left image at image + k * ifs, or null
    int rows, cols, n;
    StereoCalib cal;
    const double* poses;                // [n][16] on the host, or null
    viso_ctx* ctx;                      // the context whose device memory disp and image are (resident); null: n = 1, one host map (and
                                        // one host image) that the callee stages
    size_t px() const { return (size_t)rows * cols; }
};
// The view of a host-pointer public call, made before any check: a size that is not positive gives strides of 0.  A call without
// a calibration gets a view without a map: the callee's one null check ("non-null map and calibration") refuses either.
inline DispView disp_view_host(const int16_t* disp, const uint8_t* image, int rows, int cols, const viso_param* param, const double* pose) {
    const size_t px = rows > 0 && cols > 0 ? (size_t)rows * cols : 0;
    const StereoCalib cal = param ? StereoCalib{param->f, param->cu, param->cv, param->base} : StereoCalib{0.0, 0.0, 0.0, 0.0};
    return DispView{param ? disp : nullptr, px, image, px, rows, cols, 1, cal, pose, nullptr};
}
// speckle.hip, launch_points: the reprojection of the one map of v, on the device, at v's pose (its first three rows) or at none
int launch_points(hipStream_t s, const DispView& v, int min_disp16, float* out);
// voxelmap.hip: the opt-in voxel map (viso_map_*).  map_fuse_resident: the fuse of a resident view's maps on its context's stream;
// checks the map handle, its context and the poses
int map_fuse_resident(const char* where, viso_map* m, const DispView& v);
// tsdf.hip: the opt-in TSDF map (viso_tsdf_*).  tsdf_fuse_resident: map_fuse_resident for a TSDF map; for a gray one (tsdf_is_gray:
// 1 for a live gray map, else 0) the view has the images, for a plain one it has none
int tsdf_is_gray(viso_tsdf* t);
int tsdf_fuse_resident(const char* where, viso_tsdf* t, const DispView& v);
// the retract of a view's maps from the map ("TSDF retract"), with fuse_resident's checks; move: and their fuse at poses_new
// ([v.n][16]) behind it.  report: six words, or null
int tsdf_retract_resident(const char* where, viso_tsdf* t, const DispView& v, bool move, const double* poses_new, uint64_t* report);
// tsdf_align.hip: the opt-in frame-to-model alignment (viso_tsdf_align).  tsdf_align_resident: the alignment of a resident view's
// maps against the map, each on its own from its pose; checks the arguments, the handle and its context
int tsdf_align_resident(const char* where, viso_tsdf* t, const DispView& v, const viso_tsdf_align_params* params, viso_tsdf_alignment* records);
// the same with the photometric row ("TSDF photometric align"), from the view's images
int tsdf_align_gray_resident(const char* where, viso_tsdf* t, const DispView& v, const viso_tsdf_align_gray_params* params,
                             viso_tsdf_alignment_gray* records);
// covariance.hip: the opt-in motion covariance (viso_batch_set_covariance); one record per item, out[item], read from the item's
// X, obs, m_ptr, ld, tr, ok, n_inl, inl (what ransac_refit_kernel left)
int launch_motion_cov(hipStream_t s, const SolverItem* items_dev, int n_items, const SolverParamsDev& sp, int mode, double sigma,
                      viso_motion_cov* out);
bool motion_args_ok(int mode, double sigma_px);   // the estimators' mode 1, or mode 2 with a finite sigma_px > 0
// The direct calls viso_pose_covariance / viso_pose_refine: checks the arguments (the error names `where`), then begins the
// direct call dc and stages one SolverItem on its stream -- X, obs, inl, tr, the words ok, n_inl, m, the item, then
// rec_bytes for the record and extra_bytes for the caller's own buffers, in SLOT_GEN0.
struct PoseCall {
    DirectCall dc;
    SolverParamsDev sp;
    size_t ld;                 // max(m, 1): the item's row length
    const SolverItem* item;    // device
    char* rec;                 // device, rec_bytes
    char* extra;               // device, extra_bytes (256-byte aligned)
};
int pose_call_stage(const char* where, const double* X, const double* obs, int m, const double* tr, const int32_t* inl, int n_inl,
                    const viso_param* param, int mode, double sigma_px, const void* out, size_t rec_bytes, size_t extra_bytes,
                    PoseCall* pc);
// refine.hip: the opt-in two-frame bundle adjustment (viso_batch_set_refine); one record per item, out[item], from the item's X,
// obs, m_ptr, ld, tr, ok, n_inl, inl; pts [n_items][2][3][stride] and idx [n_items][stride] its working buffers (stride >= ld)
int launch_motion_refine(hipStream_t s, const SolverItem* items_dev, int n_items, const SolverParamsDev& sp, int mode, double sigma,
                         double* pts, int* idx, size_t stride, viso_motion_refine* out);
// window.hip: the opt-in sliding-window bundle adjustment (viso_batch_set_window_refine).  WinData: the per-frame inputs, frame F's
// X at X + F * 3 * ld, obs at obs + F * 4 * ld, inl at inl + F * ld, the cur-left / prev-left of row r at left + F * left_fs +
// r * lstride (+ 0 / + lprev); keypoint indices in [0, tab) can link.  WinWork: the working buffers (window.hip's header).
struct WinData {
    const double* X; const double* obs; const int* left; size_t left_fs; int lstride, lprev;
    const double* tr; const int* ok; const int* n_inl; const int* inl; const int* m;
    int ld, tab;
};
struct WinWork {
    int* Lp; int* nLp;   // [nf][ld] L' of every frame, [nf] its length
    int* tabs;           // [nf][2][tab] the unique row by cur-left | by prev-left (-1 none, -2 more than one)
    int* trk;            // [n_items][5][maxT] the tracks of each window
    double* pts;         // [n_items][2][3][maxT] their points (current | candidate)
    size_t maxT;         // (K - 1) ld
};
int launch_window_links(hipStream_t s, const WinData& d, const WinWork& w, int j0, int n);
int launch_window_refine(hipStream_t s, const WinData& d, const WinWork& w, const SolverParamsDev& sp, int K, int mode, double sigma,
                         int t0, int n, viso_window_record* out);
bool window_refine_args_ok(int K, int mode, double sigma_px);   // K in 2..5 and motion_args_ok
int packed_images(const char* who, const StereoImages& im);   // how many images lie back to back (extract_pack, Harris), or VISO_ERR_ARG
int launch_extract_pack(hipStream_t s, const ImageView* imgs_dev, int cap, const StereoImages& im, int extras, int r8s, int* r8cnt);
int launch_harris_response(hipStream_t s, const StereoImages& im, double k, float* resp);   // resp [images][rows][cols]
size_t harris_fused_lds(int rows, int cols, int nbinx, int nbiny, int per);
size_t harris_strip_bytes(int n_img, int rows, int cols, int nbinx, int nbiny, int per);
struct HarrisBins { int n_features, nbinx, nbiny; };   // n_features / (nbinx * nbiny) corners per bin
struct HarrisScratch { float2* tmp_kp; float* tmp_resp; int* cnt; void* part; };   // as BinArgs; part (detect): harris_strip_bytes(...) bytes, or null
struct HarrisOut { float2* kp_out; float* resp_out; int* n_out; int cap; size_t kp_stride; };   // [images][kp_stride], [images]; resp_out or null
int launch_harris_detect(hipStream_t s, const StereoImages& im, const HarrisBins& bins, double k, const HarrisScratch& tmp, const HarrisOut& out);
int launch_harris_bins(hipStream_t s, const float* resp, const StereoImages& im, const HarrisBins& bins, const HarrisScratch& tmp, const HarrisOut& out);
