// plain.hip — the plain (host-pointer) match_desc and the image cache behind it.
//
// The plain family is what the patched reference loop calls (adapters/libviso_hip.patch): per frame
//     match_desc(kp1, kp2, d1, d2)              src/viso.cpp:1240   both images new
//     match_desc(kp1, kp1_prev, d1, d1_prev)    :1264               d1 seen a moment ago, d1_prev one frame ago
//     match_desc(kp2, kp2_prev, d2, d2_prev)    :1275               the same for the right images
// so of the six (keypoints, descriptors) sets a frame passes in, four are byte for byte what an earlier call already
// brought to the device -- under another address (`d1.copyTo(d1_prev)`, :1213), so a pointer says nothing.  The context
// keeps the last PLAIN_SLOTS images resident (boundary-layout rows, bucket order, packed u16 rows, 8-bit planes) with a
// pinned host shadow of what the caller passed; an image is recognised by COMPARING its bytes with a shadow (memcmp of
// n, keypoints and descriptors: exact, no hashing), which a core does at 40-75 GB/s where the upload runs at 20-45 and
// drags sort_kp_kernel + pack_desc_kernel behind it (tools/h2d_probe.hip, profiles/r05_drop_in.txt).  A call's small
// inputs travel in ONE copy kernel's read of a pinned block, its results into a pinned mirror by copy workgroups that ride in
// the chain's next launch (common.h, OutArgs) and signal the host through a pinned word (PlainSignal) -- no copy engine, no
// synchronize; kernels that cannot have work (the other call kind's, the general path's when both images are known to
// fit the u16 rows, the wide-band stereo kernel after rectified pairs) are not launched.
#include "common.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

// ---- helper threads for the two large host-side passes of a call ---------------------------------------------------
// A miss copies the caller's 968 KB of descriptors into the slot's pinned shadow, a hit compares them with it.  One core
// does that at 10-16 GB/s when the caller's array comes from DRAM and at 40-75 GB/s from its cache.  $VISO_PLAIN_THREADS
// helpers (default 0 = none) take a slice each; they spin for a few tens of microseconds after a job and sleep on a
// condition variable otherwise.  OFF by default, measured (tools/dropin_probe.py, 201 frames): with three helpers the
// copy into the shadow is no faster (the helpers sleep between frames, waking them costs what they save) and the CALLER's
// next pass over the same array -- the loop's `d1.copyTo(d1_prev)`, src/viso.cpp:1213 -- goes from 30-40 to 65-130 us per
// frame, because slices of it now sit in other cores' caches: 1290 against 1400 frames/s.  Kept for hosts whose arrays are
// larger.  Used under the PlainLock only.
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
}
struct PlainPool {
    std::vector<std::thread> th;
    pid_t owner = getpid();           // threads do not survive fork(): a child must not wait for helpers it does not have
    std::mutex mu;
    std::condition_variable cv;
    std::atomic<unsigned long long> gen{0};
    std::atomic<int> done{0}, differ{0}, sleepers{0};
    std::atomic<bool> stop{false};
    int op = 0;                       // 0 = copy, 1 = compare
    const char* a = nullptr; char* b = nullptr; size_t bytes = 0;
    int n = 0;

    static void slice(size_t bytes, int parts, int i, size_t* lo, size_t* hi) {
        *lo = (bytes * (size_t)i / (size_t)parts) & ~(size_t)63;
        *hi = i + 1 == parts ? bytes : (bytes * (size_t)(i + 1) / (size_t)parts) & ~(size_t)63;
    }
    void work(int i) {
        size_t lo, hi;
        slice(bytes, n + 1, i, &lo, &hi);
        if (hi <= lo) return;
        if (op == 0) memcpy(b + lo, a + lo, hi - lo);
        else if (memcmp(b + lo, a + lo, hi - lo) != 0) differ.store(1, std::memory_order_relaxed);
    }
    void run(int i) {
        unsigned long long seen = 0;
        for (;;) {
            const auto t0 = std::chrono::steady_clock::now();
            while (gen.load(std::memory_order_acquire) == seen && !stop.load(std::memory_order_relaxed)) {
                cpu_relax();
                if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(60)) {
                    std::unique_lock<std::mutex> lk(mu);
                    sleepers.fetch_add(1);
                    cv.wait(lk, [&] { return gen.load(std::memory_order_acquire) != seen || stop.load(); });
                    sleepers.fetch_sub(1);
                    break;
                }
            }
            if (stop.load()) return;
            seen = gen.load(std::memory_order_acquire);
            work(i);
            done.fetch_add(1, std::memory_order_release);
        }
    }
    explicit PlainPool(int n_) : n(n_) {
        for (int i = 0; i < n; ++i) th.emplace_back([this, i] { run(i); });
    }
    ~PlainPool() {
        { std::lock_guard<std::mutex> lk(mu); stop.store(true); }
        cv.notify_all();
        for (auto& t : th) t.join();
    }
    // the caller takes the last slice; returns 1 if (op == compare and) the blocks differ
    int go(int op_, const void* src, void* dst, size_t bytes_) {
        op = op_; a = (const char*)src; b = (char*)dst; bytes = bytes_;
        done.store(0, std::memory_order_relaxed); differ.store(0, std::memory_order_relaxed);
        { std::lock_guard<std::mutex> lk(mu); gen.fetch_add(1, std::memory_order_release); }
        if (sleepers.load() > 0) cv.notify_all();
        work(n);
        while (done.load(std::memory_order_acquire) < n) cpu_relax();
        return differ.load(std::memory_order_relaxed);
    }
};
static PlainPool* g_pool = nullptr;
static bool g_pool_tried = false;
// joins the helper threads at process exit (no HIP call in there); not in a forked child, which has none to join
static struct PlainPoolReaper { ~PlainPoolReaper() { if (g_pool && g_pool->owner == getpid()) delete g_pool; g_pool = nullptr; } } g_pool_reaper;

static PlainPool* plain_pool() {
    // a process forked after the pool was made (the per-rank launchers fork BEFORE any HIP call, but a host may not) has the
    // object and none of its threads: go() would spin forever.  The child works without helpers; the parent's object is
    // leaked there on purpose (its destructor would join threads that do not exist).  $VISO_PLAIN_THREADS is not meant to be
    // combined with forked ranks.
    if (g_pool && g_pool->owner != getpid()) g_pool = nullptr;
    if (!g_pool_tried) {
        g_pool_tried = true;
        int n = 0;
        if (const char* e = getenv("VISO_PLAIN_THREADS")) n = atoi(e);
        const int hw = (int)std::thread::hardware_concurrency();
        if (hw > 0 && n > hw - 1) n = hw - 1;
        if (n > 15) n = 15;
        if (n > 0) g_pool = new PlainPool(n);
    }
    return g_pool;
}
#define PLAIN_POOL_MIN (128 * 1024)   // smaller blocks are not worth a hand-over
static void big_copy(void* dst, const void* src, size_t bytes) {
    PlainPool* p = bytes >= PLAIN_POOL_MIN ? plain_pool() : nullptr;
    if (p) p->go(0, src, dst, bytes); else if (bytes) memcpy(dst, src, bytes);
}
static bool big_equal(const void* shadow, const void* user, size_t bytes) {
    if (bytes == 0) return true;
    const size_t head = bytes < 4096 ? bytes : 4096;   // other images differ within the first bytes: no hand-over for them
    if (memcmp(shadow, user, head) != 0) return false;
    if (bytes == head) return true;
    PlainPool* p = bytes >= PLAIN_POOL_MIN ? plain_pool() : nullptr;
    if (p) return p->go(1, (const char*)user + head, (char*)shadow + head, bytes - head) == 0;
    return memcmp((const char*)shadow + head, (const char*)user + head, bytes - head) == 0;
}

#define PLAIN_SLOTS 4
#define PLAIN_DISTRUST_FRAMES 64
#define PLAIN_HDR 256      // bytes of an image's header block

// An image slot's header, in the shadow and on the device: sort_kp_kernel writes {n, bad} and the view, which pack_desc_kernel's launch reads
struct SlotHeader { int n, bad, pad[14]; ImageView view; };
static_assert(offsetof(SlotHeader, bad) == 4 && offsetof(SlotHeader, view) == 64 && sizeof(SlotHeader) <= PLAIN_HDR, "slot header");
// Offsets of a slot's pieces.  Shadow: kp | hdr | f32 rows, up to pin_end.  Device: kp | hdr | u16 rows | the aux pieces
// (16-B aligned: skp 8n + sidx 4n + rank 4n | bstart + xinfo | qord | sums | rows8), up to dev_end.
struct SlotLayout { size_t hdr, rows, pin_end, skp, sidx, rank, bstart, xinfo, qord, sums, rows8, dev_end; };
static SlotLayout slot_layout(size_t n, int dlen) {
    SlotLayout L;
    L.hdr = al256(sizeof(float2) * n); L.rows = L.hdr + PLAIN_HDR; L.pin_end = L.rows + al256(sizeof(float) * n * dlen);
    size_t o = L.rows + al256(sizeof(uint16_t) * VISO_ROW * n);
    L.skp = o; L.sidx = o + 8 * n; L.rank = o + 12 * n; o += (16 * n + 15) / 16 * 16;
    L.bstart = o; L.xinfo = o + 4 * (VISO_NB + 1); o += (4 * (VISO_NB + 1) + 32 + 15) / 16 * 16;
    L.qord = o; o += (n + 63) / 64 * 64; L.sums = o; o += (8 * n + 15) / 16 * 16;
    L.rows8 = o; L.dev_end = al256(o + VISO_ROW8 * n);
    return L;
}

struct PlainSlot {
    bool valid;
    int n, dlen, extras, r8s;
    int bad_host;                   // ImageView::bad as the host knows it: 0 / 1, -1 = not read back yet
    unsigned long long stamp;       // LRU clock
    char* pin; size_t pin_bytes;    // shadow of the caller's arrays: kp | hdr {n, bad, the ImageView} | desc
    char* dev; size_t dev_bytes;    // kp | hdr | rows | aux          (the f32 rows stay in the shadow: see plain_acquire)
    size_t o_desc, o_hdr;
    ImageView v;                    // device pointers into dev (frows: the pinned shadow)
};
// ---- the frame a stereo call opens ----------------------------------------------------------------------------------
// The reference's loop body is a fixed sequence (src/viso.cpp:1240-1313), and after the stereo call of frame t everything
// its next calls will ask for is already determined by data the library holds: the temporal calls match the two images it
// has just been given against the two of the previous stereo call (resident in their slots), collect_matches /
// triangulate_rectified read the stereo matches and the keypoints.  So the stereo call -- the one round trip the frame
// cannot avoid -- also runs those problems, in the same launches (three match_desc problems in one matcher launch, as the
// batch family does), and keeps the results.  A later call is answered from them only if its ARGUMENTS are byte for byte
// what was assumed (the images by their slots -- already a byte comparison --, match lists, x, the parameter structs by
// memcmp): the functions are pure, equal inputs give the result the direct path would compute, and any other input takes
// the direct path.  Nothing is predicted about the DATA, only about which call comes next; a wrong guess costs the
// guessed work, never a result.  $VISO_PLAIN_SPECULATE=0 / viso_plain_speculate(0) switch it off (every call direct).
#define PF_PROBS 3      // 0 = stereo (L, R), 1 = temporal (L, previous L), 2 = temporal (R, previous R)
// The frame block's counters and flags: 256 bytes at o_misc on the device, zeroed with the head by the blit in front of every
// launch, and the first 256 bytes of the pinned mirror.  Who copies what into the mirror: outA, behind the sort kernel, the words
// of the chain's first part (everything in front of n_circ) and the two images' own flags into img_bad (mirror only: on the device
// those words stay zero); outJ, behind the join kernel, the join's eight words from n_circ on.
struct FrameMisc {
    int pad0[6];
    int ovf_cnt;                  // length of the overflow queue (MatchProblem::ovf_cnt)
    int bad[2];                   // launch_match's `bad`: [0] "an image of this launch may be flagged", set in the head, read by the general kernels
                                  // (clear: they leave at once); [1] tiles match_stereo_kernel declined: it counts, match_batch_kernel<1> and the host read
    int pad1[7];
    struct { int m_cnt; int pad; unsigned long long scored; } prob[PF_PROBS];   // matches and scored pairs of problem p
    int pad2[4];
    int n_circ;                   // the join's row count
    int pad3[7];
    int img_bad[2];               // the flags of the stereo call's two images (ImageView::bad), as their pack kernels left them
    int pad4[22];
};
static_assert(sizeof(FrameMisc) == 256 && offsetof(FrameMisc, ovf_cnt) == 4 * 6 && offsetof(FrameMisc, bad) == 4 * 7 && offsetof(FrameMisc, prob) == 4 * 16 &&
              sizeof(FrameMisc::prob[0]) == 16 && offsetof(FrameMisc, prob[0].scored) == 4 * 18 && offsetof(FrameMisc, n_circ) == 4 * 32 &&
              offsetof(FrameMisc, img_bad) == 4 * 40, "the misc words stay where the kernels' pointers and the copy-outs expect them");
// The RANSAC stage's result block at o_rs (SolverItem::kept, ok, n_inl, tr, inl; RefitMirror copies it)
struct RansacOut { int kept, ok, n_inl, pad0[13]; double tr[6]; int pad1[4]; int inl[1]; };   // inl: one per row of the frame
static_assert(offsetof(RansacOut, ok) == 4 && offsetof(RansacOut, n_inl) == 8 && offsetof(RansacOut, tr) == 64 && offsetof(RansacOut, inl) == 128, "result block");
struct PlainFrame {
    bool valid;
    int L, R;                              // image slots of the stereo call
    unsigned long long sL, sR;             // their upload stamps (a recycled slot invalidates what was computed from it)
    int cap;                               // rows per problem the blocks are laid out for
    char* dev; size_t dev_bytes;
    char* host; size_t host_bytes;         // pinned mirror of the result part [o_misc, o_end)
    size_t o_misc, o_sorted[PF_PROBS], o_x, o_X, o_circ, o_xc, o_Xpc, o_rs, o_end;
    size_t o_res, o_pos, o_tile, scr_stride, o_ovf;   // device scratch behind o_end: problem p's res / pos / tile_flag at o_* + p * scr_stride; the overflow queue
    bool have[PF_PROBS], used[PF_PROBS];
    int nq[PF_PROBS], m[PF_PROBS];
    int tq[PF_PROBS], tt[PF_PROBS];
    unsigned long long stq[PF_PROBS], stt[PF_PROBS];
    viso_match_params mp[PF_PROBS];
    bool have_xX, used_x, used_X;          // collect_matches / triangulate_rectified of the stereo matches
    viso_param tri_p;
    // second part of the chain, still running when the stereo call returns: match_circle of the frame's four lists, the
    // gather of src/viso.cpp:1292-1305, ransac_minimize_reproj with the parameters / stream key the loop is expected to pass
    bool have_B, pending_B, used_circ, used_rs;
    int n_circ;                            // rows of the join (host, once B has been waited for)
    viso_param rs_p; uint64_t rs_seed, rs_frame;
    uint32_t seqJ, seqB;                   // sequence numbers of the join's copy-out (match_circle waits for this one only; the RANSAC
                                           // stage runs on) and of the RANSAC stage's copy-out
    bool pending_J;
};
struct PlainCache {
    PlainSlot slot[PLAIN_SLOTS];
    unsigned long long clock;
    long long hits, misses;
    int enabled;
    // frames: [cur] the last stereo call's, [cur ^ 1] the one before, [2] scratch of the calls outside a frame
    PlainFrame frame[3];
    int cur;
    int speculate;                         // 0 = every call direct
    bool tm_known, tm_pattern;             // temporal params seen; a temporal call fitted (L, previous L) / (R, previous R)
    viso_match_params tm;
    bool tri_known, x_pattern;             // triangulate's param seen; a collect call fitted the stereo call's outputs
    viso_param tri_p;
    bool circ_pattern;                     // a match_circle call took the frame's own lists
    unsigned long long frame_no, circ_seen_no; int circ_seen_cnt;
    bool rs_known, rs_pattern, rs_delta_stable;   // ransac's param / seed seen; the call fitted; the stream key advances regularly
    viso_param rs_p; uint64_t rs_seed, rs_last_frame, rs_delta;
    int good_streak;                       // launches in a row whose images all fitted the u16 rows
    int distrust;                          // > 0: a flagged image was seen within the last PLAIN_DISTRUST_FRAMES clean launches
    int narrow_streak;                     // stereo launches in a row in which match_stereo_kernel declined no tile (rectified pairs: always)
    long long general_reruns;
    long long spec_served[4], spec_wasted[4];   // [0] temporal match_desc, [1] collect_matches, [2] triangulate_rectified / match_circle, [3] ransac
};

// ---- the completion signal (common.h, PlainSignal; the device side is there too) -------------------------------------------
int plain_signal_next(viso_ctx* c, PlainSignal* out) {
    if (!c->sig_flag) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipHostMalloc((void**)&c->sig_flag, 256, hipHostMallocCoherent));   // fine grained: the host polls it while the kernel runs
        memset(c->sig_flag, 0, 256);
        HIP_TRY(hipMalloc((void**)&c->sig_ctr, 256));
        HIP_TRY(hipMemsetAsync(c->sig_ctr, 0, 256, c->stream));
        c->sig_seq = 0;
    }
    c->sig_seq += 1;   // unsigned: wraps after 2^32 signals, which the wait's comparison of differences allows for
    out->ctr = c->sig_ctr; out->flag = c->sig_flag; out->seq = c->sig_seq;
    return VISO_OK;
}

int plain_signal_wait(viso_ctx* c, hipStream_t s, uint32_t seq) {
    static const int off = [] { const char* e = getenv("VISO_PLAIN_SIGNAL"); return e && *e == '0'; }();   // 0: always hipStreamSynchronize (A/B aid)
    if (c->sig_flag && !off) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spin = 1;; ++spin) {
            if ((int32_t)((uint32_t)__atomic_load_n(c->sig_flag, __ATOMIC_ACQUIRE) - seq) >= 0) return VISO_OK;
            cpu_relax();
            // a signal that does not come (a failed launch, a faulting kernel): the stream knows
            if ((spin & 4095u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    return VISO_OK;
}

// ---- copy kernels: small blocks between pinned host memory and the device without the copy engine ------------------
__global__ __launch_bounds__(256) void plain_blit_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, unsigned head_words,
                                                         const int* __restrict__ n_rows, int row_words, int max_rows, PlainSignal sig) {
    unsigned total = head_words;
    if (n_rows) {
        int n = *n_rows;
        n = n < 0 ? 0 : n > max_rows ? max_rows : n;
        total += (unsigned)n * (unsigned)row_words;
    }
    const unsigned i = blockIdx.x * 1024u + threadIdx.x;   // four words per thread, 256 apart: coalesced
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned j = i + 256u * k;
        if (j < total) dst[j] = src[j];
    }
    plain_signal_done(sig, gridDim.x);
}

int plain_blit(hipStream_t s, const void* src, void* dst, size_t head_words, const int* n_rows, int row_words, int max_rows, const PlainSignal* sig) {
    size_t total = head_words + (n_rows ? (size_t)max_rows * (size_t)row_words : 0);
    if (total == 0 && sig) total = 1;   // a signal needs its kernel (the kernel copies nothing: its own bound is the device count)
    if (total == 0) return VISO_OK;
    PlainSignal g{nullptr, nullptr, 0};
    if (sig) g = *sig;
    if (total > 0x7fffffffu) { viso_set_error("plain_blit: block too large"); return VISO_ERR_UNSUPPORTED; }
    hipLaunchKernelGGL(plain_blit_kernel, dim3((unsigned)((total + 1023) / 1024)), dim3(256), 0, s,
                       reinterpret_cast<const uint32_t*>(src), reinterpret_cast<uint32_t*>(dst), (unsigned)head_words, n_rows, row_words, max_rows, g);
    HIP_TRY(hipGetLastError());
    return VISO_OK;
}

int PlainStage::flush(hipStream_t s) {
    if (off == 0) return VISO_OK;
    if (off > (1u << 20)) { HIP_TRY(hipMemcpyAsync(d, h, off, hipMemcpyHostToDevice, s)); return VISO_OK; }   // large: the copy engine is faster
    return plain_blit(s, h, d, off / 4);
}

// A grow-only block of an image slot or a frame, a quarter more than asked for: device memory (host_flags < 0) or pinned host memory.
// Replaced only behind a synchronize: a kernel of an earlier call may still use the old block.
static int plain_grow(viso_ctx* c, char** p, size_t* have, size_t need, int host_flags) {
    if (*have >= need) return VISO_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (*p) HIP_TRY(host_flags < 0 ? hipFree(*p) : hipHostFree(*p));
    *p = nullptr; *have = 0;
    need += need / 4;
    HIP_TRY(host_flags < 0 ? hipMalloc((void**)p, need) : hipHostMalloc((void**)p, need, (unsigned)host_flags));
    *have = need;
    return VISO_OK;
}

static PlainCache* plain_cache(viso_ctx* c) {
    if (!c->plain) {
        c->plain = (PlainCache*)calloc(1, sizeof(PlainCache));
        if (!c->plain) return nullptr;
        const char* e = getenv("VISO_PLAIN_CACHE");   // 0: every image is uploaded and packed again (A/B and test aid)
        c->plain->enabled = !(e && *e == '0');
        e = getenv("VISO_PLAIN_SPECULATE");
        c->plain->speculate = !(e && *e == '0');
    }
    return c->plain;
}

void plain_cache_free(viso_ctx* c) {
    if (!c->plain) return;
    for (int i = 0; i < PLAIN_SLOTS; ++i) {
        if (c->plain->slot[i].pin) (void)hipHostFree(c->plain->slot[i].pin);
        if (c->plain->slot[i].dev) (void)hipFree(c->plain->slot[i].dev);
    }
    for (int i = 0; i < 3; ++i) {
        if (c->plain->frame[i].host) (void)hipHostFree(c->plain->frame[i].host);
        if (c->plain->frame[i].dev) (void)hipFree(c->plain->frame[i].dev);
    }
    free(c->plain);
    c->plain = nullptr;
}

static void frames_forget(PlainCache* pc) {   // nothing computed ahead is handed out any more, nothing is waited for
    for (int i = 0; i < 3; ++i) { pc->frame[i].valid = false; pc->frame[i].pending_B = false; pc->frame[i].pending_J = false; }
}
// the two switches: behind the stream's work, set, and forget what was kept or learned under the old setting
static int plain_switch(const char* who, bool cache, int enable) {
    PlainLock lk;
    viso_ctx* c = viso_default_ctx();
    if (!c) return VISO_ERR_HIP;
    PlainCache* pc = plain_cache(c);
    if (!pc) { viso_set_error("%s: out of memory", who); return VISO_ERR_NOMEM; }
    HIP_TRY(hipStreamSynchronize(c->stream));
    (cache ? pc->enabled : pc->speculate) = enable != 0;
    frames_forget(pc);
    if (cache) for (int i = 0; i < PLAIN_SLOTS; ++i) pc->slot[i].valid = false;
    else pc->tm_pattern = pc->x_pattern = pc->circ_pattern = pc->rs_pattern = pc->rs_delta_stable = false;
    return VISO_OK;
}
extern "C" int viso_plain_cache(int enable) { return plain_switch("viso_plain_cache", true, enable); }
extern "C" int viso_plain_speculate(int enable) { return plain_switch("viso_plain_speculate", false, enable); }

// out[0..3] = calls answered from a frame's results (temporal match_desc, collect_matches, triangulate_rectified, -),
// out[4..7] = results computed ahead that no call asked for
extern "C" int viso_plain_speculate_stats(int64_t out[8]) {
    PlainLock lk;
    viso_ctx* c = viso_default_ctx();
    if (!c || !out) return VISO_ERR_HIP;
    PlainCache* pc = plain_cache(c);
    for (int i = 0; i < 4; ++i) { out[i] = pc ? pc->spec_served[i] : 0; out[4 + i] = pc ? pc->spec_wasted[i] : 0; }
    return VISO_OK;
}

// launches that left the general kernels out and had to be repeated with them (an image that does not fit the u16 rows
// where none was expected)
extern "C" int64_t viso_plain_general_reruns(void) {
    PlainLock lk;
    viso_ctx* c = viso_default_ctx();
    return c && c->plain ? c->plain->general_reruns : 0;
}

extern "C" int viso_plain_cache_stats(int64_t* hits, int64_t* misses) {
    PlainLock lk;
    viso_ctx* c = viso_default_ctx();
    if (!c) return VISO_ERR_HIP;
    PlainCache* pc = plain_cache(c);
    if (hits) *hits = pc ? pc->hits : 0;
    if (misses) *misses = pc ? pc->misses : 0;
    return VISO_OK;
}

// $VISO_PLAIN_TRACE=1: host microseconds of viso_match_desc by phase, summed per call kind (0 = both images resident,
// 1 / 2 = one / two uploaded), printed to stderr by viso_plain_trace_dump() (a measurement aid, tools/dropin_probe.py)
static struct PlainTrace {
    double us[3][6]; long n[3];
    double acq_us[3]; long acq_n, acq_calls;
    double srv_us[2]; long srv_n;         // temporal calls answered from the frame: [0] the two look-ups, [1] the rest
    double wait_us[2]; long wait_n[2];    // waits of the frame's later calls: [0] match_circle for the join, [1] ransac_minimize_reproj for the stage
} g_tr;
static int g_tr_on = -1;
static double tr_now() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
extern "C" void viso_plain_trace_dump(void) {
    static const char* ph[6] = {"acquire_q", "acquire_t", "setup+blit_in", "launches", "wait", "copy_out"};
    for (int k = 0; k < 3; ++k) {
        if (!g_tr.n[k]) continue;
        fprintf(stderr, "viso_match_desc, %d image(s) uploaded, %ld calls:", k, g_tr.n[k]);
        for (int j = 0; j < 6; ++j) fprintf(stderr, "  %s %.1f", ph[j], g_tr.us[k][j] / g_tr.n[k]);
        fprintf(stderr, "  (us per call)\n");
    }
    if (g_tr.acq_n) fprintf(stderr, "uploads: %ld, rows into the shadow %.1f us, pack launch %.1f us; look-ups + keypoints + sort_kp launch %.1f us per call\n", g_tr.acq_n,
                         g_tr.acq_us[0] / g_tr.acq_n, g_tr.acq_us[1] / g_tr.acq_n, g_tr.acq_us[2] / (g_tr.acq_calls > 0 ? g_tr.acq_calls : 1));
    if (g_tr.wait_n[0] || g_tr.wait_n[1])
        fprintf(stderr, "waits behind the stereo call: match_circle for the join %.1f us (%ld), ransac_minimize_reproj for the stage %.1f us (%ld)\n",
                g_tr.wait_n[0] ? g_tr.wait_us[0] / g_tr.wait_n[0] : 0.0, g_tr.wait_n[0], g_tr.wait_n[1] ? g_tr.wait_us[1] / g_tr.wait_n[1] : 0.0, g_tr.wait_n[1]);
    if (g_tr.srv_n) fprintf(stderr, "temporal calls answered from the frame: %ld, look-ups (byte comparison of both images) %.1f us, the rest %.1f us\n", g_tr.srv_n, g_tr.srv_us[0] / g_tr.srv_n, g_tr.srv_us[1] / g_tr.srv_n);
    g_tr = PlainTrace{};
}

// The slot that holds (kp, d), found by comparing bytes; -1: not resident.
static int plain_lookup(PlainCache* pc, const float* kp, const float* d, int n, int dlen, int extras, int r8s) {
    const size_t kb = sizeof(float2) * (size_t)n, db = sizeof(float) * (size_t)n * dlen;
    if (pc->enabled)
        for (int i = 0; i < PLAIN_SLOTS; ++i) {
            PlainSlot& s = pc->slot[i];
            if (!s.valid || s.n != n || s.dlen != dlen || s.extras != extras || s.r8s != r8s) continue;
            if ((kb && memcmp(s.pin, kp, kb) != 0) || !big_equal(s.pin + s.o_desc, d, db)) continue;
            pc->hits += 1;   // the stamp stays the upload's: slots are recycled oldest UPLOAD first.  (Refreshed on a hit -- LRU --
            return i;        // the loop's own order evicts frame t-1's left image when frame t's arrives: its last use was the
        }                    // temporal-left call, before the right images' -- and the temporal calls of frame t upload it again.)
    pc->misses += 1;
    return -1;
}

// An image that is not resident comes to the device in two pieces.  Keypoints + header (16 KB): sort_kp_kernel fetches them
// from the pinned shadow itself (KpImport) -- plain_prepare picks the slot (`keep`, `keep2`: slots that must not be evicted, the
// call's other image; -1 for none), copies the keypoints into the shadow and fills the import.  The f32 descriptor rows
// (968 KB) are read ONCE, by pack_desc_kernel, which turns them into the u16 rows the matchers use: it reads them straight
// from the shadow over PCIe -- no copy-engine transfer (25 us on the wire + 20 us of host time in hipMemcpyAsync per image,
// and every kernel of the call queued behind both) and no second copy of the rows in device memory; plain_finish copies
// them into the shadow and launches that kernel.  A call's order: prepare both images, ONE sort_kp launch for what is new
// (it needs the keypoints only and runs while the host copies rows), then rows + pack launch image by image, so that the
// GPU packs the first image while the host copies the second.  (Only the general path reads f32 rows again -- images
// with non-integer descriptors -- and then from the shadow: slow, correct.)
static int plain_prepare(viso_ctx* c, PlainCache* pc, const float* kp, int n, int dlen, int extras, int r8s, int keep, int keep2, KpImport* imp) {
    const size_t kb = sizeof(float2) * (size_t)n;
    int vi = -1;   // an empty slot, else the one uploaded longest ago
    for (int i = 0; i < PLAIN_SLOTS && vi < 0; ++i)
        if (i != keep && i != keep2 && !pc->slot[i].valid) vi = i;
    for (int i = 0; i < PLAIN_SLOTS && (vi < 0 || pc->slot[vi].valid); ++i)
        if (i != keep && i != keep2 && (vi < 0 || pc->slot[i].stamp < pc->slot[vi].stamp)) vi = i;
    PlainSlot& s = pc->slot[vi];
    s.valid = false;
    const SlotLayout L = slot_layout((size_t)(n > 0 ? n : 1), dlen);
    int r;
    if ((r = plain_grow(c, &s.pin, &s.pin_bytes, L.pin_end, hipHostMallocDefault)) < 0 || (r = plain_grow(c, &s.dev, &s.dev_bytes, L.dev_end, -1)) < 0) return r;
    if (kb) memcpy(s.pin, kp, kb);
    SlotHeader *hdr = reinterpret_cast<SlotHeader*>(s.pin + L.hdr), *dhdr = reinterpret_cast<SlotHeader*>(s.dev + L.hdr);
    ImageView v{};
    v.kp = reinterpret_cast<const float2*>(s.dev); v.frows = reinterpret_cast<const float*>(s.pin + L.rows);
    v.n = &dhdr->n; v.bad = &dhdr->bad; v.rows = reinterpret_cast<uint16_t*>(s.dev + L.rows);
    v.skp = reinterpret_cast<float2*>(s.dev + L.skp); v.sidx = reinterpret_cast<int*>(s.dev + L.sidx); v.rank = reinterpret_cast<int*>(s.dev + L.rank);
    v.bstart = reinterpret_cast<int*>(s.dev + L.bstart); v.xinfo = reinterpret_cast<float*>(s.dev + L.xinfo);
    v.qord = reinterpret_cast<uint8_t*>(s.dev + L.qord); v.sums = reinterpret_cast<uint2*>(s.dev + L.sums); v.rows8 = reinterpret_cast<uint8_t*>(s.dev + L.rows8);
    hdr->n = n; hdr->bad = dlen > VISO_ROW ? 1 : 0;   // rows that do not fit the packed format: the image takes the general path
    hdr->view = v;
    // sort_kp_kernel gets the image's view in its arguments, writes the header words {n, bad} and leaves a copy of the view on
    // the device where pack_desc_kernel's launch finds it (the copy kernel that used to bring keypoints + header over first is gone)
    *imp = KpImport{}; imp->src_kp = reinterpret_cast<const float2*>(s.pin); imp->n = n; imp->bad0 = hdr->bad;
    imp->view_dst = &dhdr->view; imp->view = v;
    s.n = n; s.dlen = dlen; s.extras = extras; s.r8s = r8s;
    s.bad_host = dlen > VISO_ROW ? 1 : -1;
    s.o_desc = L.rows; s.o_hdr = L.hdr; s.v = v;
    return vi;
}

static int plain_finish(viso_ctx* c, PlainCache* pc, int vi, const float* d, hipStream_t stream) {
    PlainSlot& s = pc->slot[vi];
    const int n = s.n, dlen = s.dlen;
    const double ta0 = g_tr_on > 0 ? tr_now() : 0;
    // (the rows in two parts, the first packed while the second is copied -- halves in round 5: 2 356 against 2 337 frames/s; 5/8 + 3/8
    // of the call's last image in round 6: 2 929 against 2 932, four alternating runs each -- one more launch on the host for a few us
    // less of the GPU's chain: inside the noise both times; not kept)
    big_copy(s.pin + s.o_desc, d, sizeof(float) * (size_t)n * dlen);
    const double ta1 = g_tr_on > 0 ? tr_now() : 0;
    int r;
    const ImageView* dview = &reinterpret_cast<const SlotHeader*>(s.dev + s.o_hdr)->view;
    if (dlen <= VISO_ROW && (r = launch_pack(stream, dview, 1, n > 0 ? n : 1, dlen, nullptr, const_cast<int*>(s.v.bad), s.extras, s.r8s, nullptr)) < 0) return r;
    if (g_tr_on > 0) { g_tr.acq_us[0] += ta1 - ta0; g_tr.acq_us[1] += tr_now() - ta1; g_tr.acq_n += 1; }
    s.stamp = ++pc->clock;
    s.valid = true;
    return VISO_OK;
}

// a copy-out (common.h, OutArgs) as a kernel of its own: where the chain has no next kernel for it to ride in
__global__ __launch_bounds__(256) void plain_out_kernel(OutArgs a) { plain_out_blocks(a, blockIdx.x); }

static bool params_equal(const viso_match_params& a, const viso_match_params& b) {
    return a.enforce_epipolar == b.enforce_epipolar && a.enforce_2nd_best == b.enforce_2nd_best && a.max_neighbors == b.max_neighbors &&
           memcmp(a.F, b.F, sizeof(a.F)) == 0 && memcmp(&a.sampson_thresh, &b.sampson_thresh, 8) == 0 &&
           memcmp(&a.ratio_2nd_best, &b.ratio_2nd_best, 8) == 0 && memcmp(&a.radius, &b.radius, 8) == 0;
}
static bool tri_equal(const viso_param& a, const viso_param& b) {   // the fields triangulate_rectified reads, bit for bit
    return memcmp(&a.base, &b.base, 8) == 0 && memcmp(&a.f, &b.f, 8) == 0 && memcmp(&a.cu, &b.cu, 8) == 0 && memcmp(&a.cv, &b.cv, 8) == 0;
}

struct FrameHead { MatchProblem p[PF_PROBS]; TriItem tri; SolverItem rs; OutArgs outA, outJ; };

// A frame's block by its offset (o_X, or offsetof(FrameHead, ...)): on the device, and in the pinned mirror, which holds [o_misc, o_end)
template <class T> static T* frame_dev(const PlainFrame& f, size_t off) { return reinterpret_cast<T*>(f.dev + off); }
template <class T> static T* frame_host(const PlainFrame& f, size_t off) { return reinterpret_cast<T*>(f.host + (off - f.o_misc)); }
static size_t frame_ld(const PlainFrame& f) { return (size_t)(f.cap > 0 ? f.cap : 1); }   // leading dimension of the column blocks (x, X, xc, Xpc)
static const int* frame_rows(const PlainFrame& f, int p) { return frame_host<const int>(f, f.o_sorted[p]); }

// lays a frame's blocks out for `cap` rows per problem (grow only)
static int frame_reserve(viso_ctx* c, PlainFrame& f, int cap) {
    const size_t C = (size_t)(cap > 0 ? cap : 1);
    size_t o = al256(sizeof(FrameHead));
    f.o_misc = o; o += sizeof(FrameMisc);
    for (int p = 0; p < PF_PROBS; ++p) { f.o_sorted[p] = o; o += al256(sizeof(int) * 3 * C); }
    f.o_x = o; o += al256(sizeof(double) * 4 * C); f.o_X = o; o += al256(sizeof(double) * 3 * C);
    f.o_circ = o; o += al256(sizeof(int) * 6 * C);
    f.o_xc = o; o += al256(sizeof(double) * 4 * C); f.o_Xpc = o; o += al256(sizeof(double) * 3 * C);
    f.o_rs = o; o += offsetof(RansacOut, inl) + al256(sizeof(int) * C);
    f.o_end = o;
    // behind the mirrored part, scratch of the matchers: res | pos | tile_flag per problem, then the overflow queue they share
    f.o_res = o; f.o_pos = f.o_res + al256(sizeof(int2) * C); f.o_tile = f.o_pos + al256(sizeof(int) * C);
    f.scr_stride = f.o_tile + al256(sizeof(int) * (C / 64 + 1)) - f.o_res;
    f.o_ovf = f.o_res + PF_PROBS * f.scr_stride;
    int r = plain_grow(c, &f.dev, &f.dev_bytes, f.o_ovf + al256(sizeof(int2) * PF_PROBS * C), -1);
    // the mirror is coherent memory: the host reads it right behind the signal, possibly before the kernel has retired
    if (r < 0 || (r = plain_grow(c, &f.host, &f.host_bytes, f.o_end - f.o_misc, hipHostMallocCoherent)) < 0) return r;
    f.cap = cap;
    return VISO_OK;
}

static void frame_reset(PlainFrame& f) {
    f.valid = false;
    for (int p = 0; p < PF_PROBS; ++p) { f.have[p] = f.used[p] = false; f.m[p] = 0; }
    f.have_xX = f.used_x = f.used_X = f.have_B = f.used_circ = f.used_rs = false;
    f.n_circ = 0;
}

// Waits for the second part of a frame's chain.  stage 0: the join and the gathered columns are in the mirror (match_circle waits for this
// one only, the RANSAC stage runs on); stage 1: the RANSAC result is too -- the chain's last kernel: everything before it on the stream is done
static int frame_wait(viso_ctx* c, PlainFrame& f, int stage) {
    if (!(stage ? f.pending_B : f.pending_J)) return VISO_OK;
    const double tw0 = g_tr_on > 0 ? tr_now() : 0;
    const int r = plain_signal_wait(c, c->stream, stage ? f.seqB : f.seqJ);
    if (r < 0) return r;
    if (g_tr_on > 0) { g_tr.wait_us[stage] += tr_now() - tw0; g_tr.wait_n[stage] += 1; }
    if (stage) f.pending_B = false;
    f.pending_J = false;
    f.n_circ = frame_host<const FrameMisc>(f, f.o_misc)->n_circ;
    return VISO_OK;
}

// what a frame computed ahead and nobody asked for: the pattern it was guessed from no longer holds
static void frame_retire(PlainCache* pc, PlainFrame& f) {
    if (!f.valid) return;
    if ((f.have[1] && !f.used[1]) || (f.have[2] && !f.used[2])) { pc->tm_pattern = false; pc->spec_wasted[0] += 1; }
    if (f.have_xX && !f.used_x) { pc->x_pattern = false; pc->spec_wasted[1] += 1; }
    if (f.have_xX && f.used_x && !f.used_X) pc->spec_wasted[2] += 1;
    if (f.have_B && !f.used_circ) { pc->circ_pattern = false; pc->spec_wasted[2] += 1; }
    if (f.have_B && !f.used_rs) { pc->rs_pattern = false; pc->spec_wasted[3] += 1; }
}

// An error return must not leave work in flight: the kernels queued so far (copy, sort_kp, pack -- possibly on the side
// stream) read the slots' pinned shadows and the context's pinned block, a slot may already be marked valid although its
// pack kernel never ran to the end, and the next call would memcpy over a shadow a queued kernel is still pulling over
// PCIe, or get a byte-comparison hit on half-packed rows.  So: wait for both streams, forget every image and every frame.
// (Errors here are HIP failures; nothing is optimised for them.)
static void plain_quiesce(viso_ctx* c, PlainCache* pc) {
    (void)hipStreamSynchronize(c->stream);
    for (int i = 0; i < PLAIN_SLOTS; ++i) pc->slot[i].valid = false;
    frames_forget(pc);
    pc->good_streak = pc->narrow_streak = 0;
}

// ---- one launch of a frame: match_run drives the five stages below over this plan -------------------------------------
struct FramePlan {
    int iq, it, n1, dlen, variant, extras, r8s;   // the call (match_desc_locked): its images' slots, its queries, what the rows were packed for
    const viso_match_params* mp; bool stereo, force_general;   // ... its parameters; a stereo call; the repeated launch: every kernel is in it
    PlainFrame* f;                                // frame_open: the object that takes the call,
    int np, cap;                                  //   its problems (1, or 3: the temporal calls ride along) and rows per problem,
    bool spec_x, spec_B;                          //   collect + triangulate ride in the sort kernel / the second part (join, RANSAC) follows,
    int saved_cur; unsigned long long saved_no;   //   what a repeated launch puts back
    FrameHead* H;                                 // frame_fill_head: the head in the context's pinned block,
    bool need_general;                            //   whether the launch includes the general kernels,
    int *rs_tab, *rs_queue, rs_tabn;              //   the second part's join table and hypothesis queue
    uint32_t seqA;                                // frame_copy_outs: the signal of the first copy-out
    bool skip_wide;                               // frame_queue_first: the wide-band stereo kernel was left out
};

// stage 1: which frame object takes the call, which problems ride along, where its blocks lie
static int frame_open(viso_ctx* c, PlainCache* pc, FramePlan& P) {
    int r;
    const int iq = P.iq, it = P.it, dlen = P.dlen;
    P.saved_cur = pc->cur; P.saved_no = pc->frame_no;
    PlainFrame* f = &pc->frame[2];
    P.np = 1; P.spec_x = P.spec_B = false;
    if (P.stereo && pc->speculate) {
        if ((r = frame_wait(c, pc->frame[pc->cur ^ 1], 1)) < 0) return r;
        // The frame that leaves is the one before the last stereo call's: every call that could have used its results is over,
        // so what it computed ahead and nobody asked for is known now, whatever becomes of THIS launch (a repeated launch finds
        // the object reset -- not valid -- and counts nothing twice)
        frame_retire(pc, pc->frame[pc->cur ^ 1]);
        pc->frame_no += 1; pc->cur ^= 1;
        f = &pc->frame[pc->cur];
        const PlainFrame& prv = pc->frame[pc->cur ^ 1];
        frame_reset(*f);
        f->L = iq; f->R = it; f->sL = pc->slot[iq].stamp; f->sR = pc->slot[it].stamp;
        if (pc->tm_known && pc->tm_pattern && prv.valid && iq != it && prv.L != prv.R &&
            pc->slot[prv.L].valid && pc->slot[prv.L].stamp == prv.sL && pc->slot[prv.R].valid && pc->slot[prv.R].stamp == prv.sR &&
            pc->slot[prv.L].dlen == dlen && pc->slot[prv.R].dlen == dlen && pc->slot[prv.L].extras == P.extras && pc->slot[prv.R].extras == P.extras &&
            pc->slot[prv.L].r8s == P.r8s && pc->slot[prv.R].r8s == P.r8s && prv.L != iq && prv.L != it && prv.R != iq && prv.R != it)
            P.np = 3;
        P.spec_x = pc->tri_known && pc->x_pattern;
        P.spec_B = P.np == 3 && P.spec_x && prv.have_xX && prv.have[0] && pc->circ_pattern && pc->rs_known && pc->rs_pattern && pc->rs_delta_stable &&
                   pc->rs_p.ransac_iter >= 1 && pc->rs_p.ransac_iter <= 4096;
    } else frame_reset(*f);
    P.f = f;
    const PlainSlot &sq = pc->slot[iq], &st = pc->slot[it];
    f->have[0] = true; f->nq[0] = P.n1; f->tq[0] = iq; f->tt[0] = it; f->stq[0] = sq.stamp; f->stt[0] = st.stamp; f->mp[0] = *P.mp;
    if (P.np == 3) {
        const PlainFrame& prv = pc->frame[pc->cur ^ 1];
        f->have[1] = true; f->nq[1] = sq.n; f->tq[1] = iq; f->tt[1] = prv.L; f->stq[1] = sq.stamp; f->stt[1] = prv.sL; f->mp[1] = pc->tm;
        f->have[2] = true; f->nq[2] = st.n; f->tq[2] = it; f->tt[2] = prv.R; f->stq[2] = st.stamp; f->stt[2] = prv.sR; f->mp[2] = pc->tm;
    }
    P.cap = P.n1;
    for (int p = 1; p < P.np; ++p) P.cap = f->nq[p] > P.cap ? f->nq[p] : P.cap;
    return frame_reserve(c, *f, P.cap);
}

// stage 2: the head of the frame's block in the context's pinned block -- problems, TriItem, SolverItem, zeroed counters: ONE copy in
static int frame_fill_head(viso_ctx* c, PlainCache* pc, FramePlan& P) {
    int r; char* hin;
    PlainFrame& f = *P.f;
    const PlainSlot &sq = pc->slot[P.iq], &st = pc->slot[P.it];
    if ((r = ctx_pinned(c, 0, f.o_misc + sizeof(FrameMisc), &hin)) < 0) return r;
    P.H = reinterpret_cast<FrameHead*>(hin);
    FrameMisc* hmisc = reinterpret_cast<FrameMisc*>(hin + f.o_misc);
    FrameMisc* dmisc = frame_dev<FrameMisc>(f, f.o_misc);
    memset(hmisc, 0, sizeof(FrameMisc));
    // The general (float / double) kernels are for images whose descriptors do not fit the u16 rows.  Whether a NEW image
    // does is known only after its pack kernel has run; once a few launches in a row have seen none, new images are expected
    // to fit and the three general kernels are left out of the launch (15 us of the chain).  If the expectation fails
    // -- the images' own flags come back with the results -- sort_matches_kernel has emitted EMPTY lists for the problems
    // concerned (flagged_empty) and the call is repeated with the general kernels: same results, later.
    bool any_bad = false, any_unknown = false;
    for (int p = 0; p < P.np; ++p) {
        const PlainSlot &a = pc->slot[f.tq[p]], &b = pc->slot[f.tt[p]];
        if (a.bad_host == 1 || b.bad_host == 1) any_bad = true;
        if (a.bad_host < 0 || b.bad_host < 0) any_unknown = true;
        MatchProblem M{};
        M.q = a.v; M.t = b.v;
        M.res = frame_dev<int2>(f, f.o_res + p * f.scr_stride); M.pos = frame_dev<int>(f, f.o_pos + p * f.scr_stride);
        M.tile_flag = frame_dev<int>(f, f.o_tile + p * f.scr_stride); M.sorted = frame_dev<int>(f, f.o_sorted[p]);
        M.m_cnt = &dmisc->prob[p].m_cnt; M.scored = &dmisc->prob[p].scored;
        M.pidx = p == 0 ? 0 : 1; M.cap = P.cap;
        M.ovf = frame_dev<int2>(f, f.o_ovf); M.ovf_cnt = &dmisc->ovf_cnt;
        P.H->p[p] = M;
    }
    // A source that has produced a flagged image lately keeps the general kernels in the launch: a stream with sporadic
    // fractional images would otherwise pay a dropped launch + a full synchronize + a second launch on every such frame
    const bool trust = pc->good_streak >= 2 && !P.force_general && pc->distrust == 0;
    P.need_general = any_bad || (any_unknown && !trust) || P.dlen > VISO_ROW;
    if (P.need_general) hmisc->bad[0] = 1;   // the general kernels' early-exit hint; they look at every image's own flag
    if (P.spec_x) {
        TriItem T{};
        T.kp1 = sq.v.kp; T.kp2 = st.v.kp; T.match = frame_dev<const int>(f, f.o_sorted[0]); T.m_cnt = &dmisc->prob[0].m_cnt;
        T.x = frame_dev<double>(f, f.o_x); T.X = frame_dev<double>(f, f.o_X); T.ld = (int)frame_ld(f);
        P.H->tri = T;
    }
    if (P.spec_B) {
        const int iters = pc->rs_p.ransac_iter;
        double* dtrh; int* dhyp; char* drot;
        P.rs_tabn = sq.n > st.n ? sq.n : st.n;
        if (pc->slot[pc->frame[pc->cur ^ 1].L].n > P.rs_tabn) P.rs_tabn = pc->slot[pc->frame[pc->cur ^ 1].L].n;
        if ((r = ctx_scratch(c, SLOT_CIRCLE_TAB, sizeof(int) * 3 * (size_t)(P.rs_tabn + 1), (void**)&P.rs_tab)) < 0) return r;
        if ((r = ctx_scratch(c, SLOT_HYP_WORDS, sizeof(int) * (4 + 2 * (size_t)iters), (void**)&dhyp)) < 0) return r;
        if ((r = ctx_scratch(c, SLOT_HYP_TR, sizeof(double) * 6 * (size_t)(iters + 1), (void**)&dtrh)) < 0) return r;
        if ((r = ctx_scratch(c, SLOT_RANSAC_QUEUE, sizeof(int) * (2 + 4 * (size_t)iters + 3), (void**)&P.rs_queue, true)) < 0) return r;
        if ((r = ctx_scratch(c, SLOT_RANSAC_ROT, viso_rot_bytes(iters), (void**)&drot)) < 0) return r;
        f.rs_p = pc->rs_p; f.rs_seed = pc->rs_seed; f.rs_frame = pc->rs_last_frame + pc->rs_delta;
        RansacOut* rso = frame_dev<RansacOut>(f, f.o_rs);
        SolverItem S{};
        S.X = frame_dev<const double>(f, f.o_Xpc); S.obs = frame_dev<const double>(f, f.o_xc);
        S.m_ptr = &dmisc->n_circ; S.ld = (int)frame_ld(f); S.samples = nullptr; S.samp_h = P.rs_queue + 2 + iters; S.frame = f.rs_frame;
        S.tr_h = dtrh; S.ok_h = dhyp; S.cnt_h = dhyp + iters; S.rot = drot;
        S.kept = &rso->kept; S.ok = &rso->ok; S.n_inl = &rso->n_inl; S.tr = rso->tr; S.inl = rso->inl;
        P.H->rs = S;
    }
    return VISO_OK;
}

static void out_add(OutArgs& o, const void* src, void* dst, const int* cnt, int row_words, int max_rows) {
    OutRegion& R = o.r[o.n_regions++];
    R.src = static_cast<const uint32_t*>(src); R.dst = static_cast<uint32_t*>(dst); R.cnt = cnt; R.row_words = row_words; R.max_rows = max_rows;
}
static void out_block(OutArgs& o, const PlainFrame& f, size_t off, const int* cnt, int row_words, int max_rows) {   // a block of the frame to its place in the mirror
    out_add(o, frame_dev<char>(f, off), frame_host<char>(f, off), cnt, row_words, max_rows);
}

// stage 3: the copy-outs into the frame's pinned mirror (common.h, OutArgs): the lists (and x, X) behind the sort kernel -- riding in
// the join kernel's launch when the frame has one, a kernel of their own otherwise; the join and the gathered columns behind
// the join kernel, riding in ransac_coop_kernel's launch.  Each signals: match_circle returns as soon as the join is there,
// the RANSAC stage runs on behind the caller's gather loop.  FrameMisc says which of its words each of the two owns.
static int frame_copy_outs(viso_ctx* c, PlainCache* pc, FramePlan& P) {
    int r;
    PlainFrame& f = *P.f;
    const size_t C = frame_ld(f);
    FrameMisc* dmisc = frame_dev<FrameMisc>(f, f.o_misc);
    FrameMisc* omisc = frame_host<FrameMisc>(f, f.o_misc);
    const int* m0 = &dmisc->prob[0].m_cnt;
    OutArgs& oa = P.H->outA = OutArgs{};
    out_block(oa, f, f.o_misc, nullptr, offsetof(FrameMisc, n_circ) / 4, 1);
    out_add(oa, pc->slot[P.iq].v.bad, &omisc->img_bad[0], nullptr, 1, 1);
    out_add(oa, pc->slot[P.it].v.bad, &omisc->img_bad[1], nullptr, 1, 1);
    for (int p = 0; p < P.np; ++p) out_block(oa, f, f.o_sorted[p], &dmisc->prob[p].m_cnt, 3, f.nq[p]);
    if (P.spec_x) {
        for (int k = 0; k < 4; ++k) out_block(oa, f, f.o_x + sizeof(double) * C * k, m0, 2, P.n1);
        for (int k = 0; k < 3; ++k) out_block(oa, f, f.o_X + sizeof(double) * C * k, m0, 2, P.n1);
    }
    const size_t tpb = P.spec_B ? 1024 : 256;   // threads of the workgroups that will do it: four words each
    oa.gx = (int)((3 * C + 4 * tpb - 1) / (4 * tpb));
    if ((r = plain_signal_next(c, &oa.sig)) < 0) return r;
    P.seqA = oa.sig.seq;
    if (P.spec_B) {
        OutArgs& oj = P.H->outJ = OutArgs{};
        out_block(oj, f, f.o_misc + offsetof(FrameMisc, n_circ), nullptr, (offsetof(FrameMisc, img_bad) - offsetof(FrameMisc, n_circ)) / 4, 1);
        out_block(oj, f, f.o_circ, &dmisc->n_circ, 6, P.cap);
        for (int k = 0; k < 4; ++k) out_block(oj, f, f.o_xc + sizeof(double) * C * k, &dmisc->n_circ, 2, P.cap);
        for (int k = 0; k < 3; ++k) out_block(oj, f, f.o_Xpc + sizeof(double) * C * k, &dmisc->n_circ, 2, P.cap);
        oj.gx = (int)((6 * C + 1023) / 1024);
        if ((r = plain_signal_next(c, &oj.sig)) < 0) return r;
        f.seqJ = oj.sig.seq;
    }
    return VISO_OK;
}

// stage 4, first part: the matchers and the sort kernel
static int frame_queue_first(viso_ctx* c, PlainCache* pc, FramePlan& P) {
    int r;
    PlainFrame& f = *P.f;
    FrameMisc* dmisc = frame_dev<FrameMisc>(f, f.o_misc);
    const MatchProblem* dprob = frame_dev<const MatchProblem>(f, offsetof(FrameHead, p));
    MatchParamsDev mpd[2]; fill_match_params(&mpd[0], P.mp);
    if (P.np == 3) fill_match_params(&mpd[1], &pc->tm); else mpd[1] = mpd[0];
    int kinds = P.np == 3 ? VISO_KIND_ALL : P.stereo ? VISO_KIND_STEREO : VISO_KIND_TEMPORAL;
    // match_batch_kernel<1> takes the tiles whose epipolar band match_stereo_kernel finds too wide (pairs that are not
    // rectified): after a few stereo launches without such a tile it is left out (5 us of the chain the caller waits for);
    // the number of declined tiles comes back with the results, and a launch that had one without the kernel is repeated
    P.skip_wide = P.stereo && pc->narrow_streak >= 2 && !P.force_general;
    if (P.skip_wide) kinds |= VISO_KIND_NO_WIDE;
    if ((r = launch_match(c->stream, dprob, P.np, P.cap, P.dlen, mpd, dmisc->bad, nullptr, nullptr, 0, P.variant, frame_dev<const int2>(f, f.o_ovf),
                                &dmisc->ovf_cnt, P.r8s, P.need_general ? 1 : 0, kinds)) < 0) return r;
    if (!P.spec_x) return launch_sort(c->stream, dprob, P.np, P.cap, P.need_general ? 0 : 1);
    SolverParamsDev sp; fill_solver_params(&sp, &pc->tri_p);   // collect_matches / triangulate_rectified of the stereo list ride in the sort kernel
    return launch_sort(c->stream, dprob, P.np, P.cap, P.need_general ? 0 : 1, frame_dev<const TriItem>(f, offsetof(FrameHead, tri)), &sp);
}

// stage 4, second part: the join and the RANSAC stage -- they keep running while the caller goes through its next calls
static int frame_queue_second(viso_ctx* c, PlainCache* pc, FramePlan& P) {
    int r;
    PlainFrame& f = *P.f;
    const PlainFrame& prv = pc->frame[pc->cur ^ 1];
    FrameMisc* dmisc = frame_dev<FrameMisc>(f, f.o_misc);
    const FrameMisc* pmisc = frame_dev<const FrameMisc>(prv, prv.o_misc);
    CircleArgs ca{};
    ca.lr = frame_dev<const int>(f, f.o_sorted[0]); ca.lrp = frame_dev<const int>(prv, prv.o_sorted[0]);
    ca.m11 = frame_dev<const int>(f, f.o_sorted[1]); ca.m22 = frame_dev<const int>(f, f.o_sorted[2]);
    ca.n_lr_p = &dmisc->prob[0].m_cnt; ca.n_lrp_p = &pmisc->prob[0].m_cnt; ca.n11_p = &dmisc->prob[1].m_cnt; ca.n22_p = &dmisc->prob[2].m_cnt;
    ca.rows = frame_dev<int>(f, f.o_circ); ca.cap = P.cap; ca.out_n = &dmisc->n_circ;
    // x_c / Xp_c of :1292-1305 come out of the join kernel's tail (no gather kernel of their own)
    ca.g_x = frame_dev<const double>(f, f.o_x); ca.g_ldx = (int)frame_ld(f);
    ca.g_Xp = frame_dev<const double>(prv, prv.o_X); ca.g_ldXp = (int)frame_ld(prv);
    ca.g_xc = frame_dev<double>(f, f.o_xc); ca.g_Xpc = frame_dev<double>(f, f.o_Xpc); ca.g_ldc = (int)frame_ld(f);
    ca.ride = frame_dev<const OutArgs>(f, offsetof(FrameHead, outA)); ca.ride_blocks = P.H->outA.n_regions * P.H->outA.gx;
    if ((r = launch_circle_table(c->stream, ca, P.rs_tab, P.rs_tabn)) < 0) return r;
    SolverParamsDev sp; fill_solver_params(&sp, &f.rs_p);
    RefitMirror rm{};   // the pose and the inliers go into the mirror from the refit kernel itself, which signals
    const RansacOut* rso = frame_dev<const RansacOut>(f, f.o_rs); RansacOut* rsh = frame_host<RansacOut>(f, f.o_rs);
    rm.res_src = reinterpret_cast<const uint32_t*>(rso); rm.res_dst = reinterpret_cast<uint32_t*>(rsh); rm.res_words = offsetof(RansacOut, inl) / 4;
    rm.n_inl = &rso->n_inl; rm.inl_src = reinterpret_cast<const uint32_t*>(rso->inl); rm.inl_dst = reinterpret_cast<uint32_t*>(rsh->inl); rm.max_inl = P.cap;
    if ((r = plain_signal_next(c, &rm.sig)) < 0) return r;
    f.seqB = rm.sig.seq;
    if ((r = launch_ransac(c->stream, frame_dev<const SolverItem>(f, offsetof(FrameHead, rs)), 1, f.rs_p.ransac_iter, f.rs_seed, sp,
                           P.rs_queue, c->gn_split ? c->gn_split : 1, P.cap, &rm,
                           frame_dev<const OutArgs>(f, offsetof(FrameHead, outJ)), P.H->outJ.n_regions * P.H->outJ.gx)) < 0) return r;
    f.have_B = true; f.pending_B = true; f.pending_J = true;
    return VISO_OK;
}

// The launch lacked a kernel that turned out to have work: everything it produced is dropped, the call repeated with it
#define PLAIN_RERUN 2
static int frame_repeat(viso_ctx* c, PlainCache* pc, FramePlan& P) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    P.f->pending_B = P.f->pending_J = false; frame_reset(*P.f);
    pc->cur = P.saved_cur; pc->frame_no = P.saved_no;
    pc->general_reruns += 1;
    return PLAIN_RERUN;
}

// stage 5: behind the first copy-out's signal -- the counts, what the launch learned about its images and its stereo pair, the stereo list
static int frame_harvest(viso_ctx* c, PlainCache* pc, FramePlan& P, int32_t* out_match, int* out_n) {
    PlainFrame& f = *P.f;
    PlainSlot &sq = pc->slot[P.iq], &st = pc->slot[P.it];
    const FrameMisc* omisc = frame_host<const FrameMisc>(f, f.o_misc);
    for (int p = 0; p < P.np; ++p) {
        const int m = omisc->prob[p].m_cnt;
        if (m < 0 || m > f.nq[p]) { frame_reset(f); viso_set_error("viso_match_desc: device returned %d matches for %d queries", m, f.nq[p]); return VISO_ERR_HIP; }
        f.m[p] = m;
    }
    if (P.stereo) {   // tiles the stereo kernel left to the wide-band kernel
        pc->narrow_streak = omisc->bad[1] == 0 ? pc->narrow_streak + 1 : 0;
        if (omisc->bad[1] != 0 && P.skip_wide) return frame_repeat(c, pc, P);   // ... which was not in the launch
    }
    sq.bad_host = omisc->img_bad[0] != 0; st.bad_host = omisc->img_bad[1] != 0;   // the images' own flags, as their pack kernels left them
    if (sq.bad_host || st.bad_host) {
        pc->good_streak = 0; pc->distrust = PLAIN_DISTRUST_FRAMES;
        if (!P.need_general) return frame_repeat(c, pc, P);   // unexpected: the launch had no kernel for them
    } else {
        pc->good_streak += 1;
        if (pc->distrust > 0) pc->distrust -= 1;
    }
    if (f.m[0] > 0) memcpy(out_match, frame_rows(f, 0), sizeof(int) * 3 * (size_t)f.m[0]);
    f.valid = P.stereo && pc->speculate;
    f.have_xX = P.spec_x; f.tri_p = pc->tri_p;
    *out_n = f.m[0];
    return VISO_OK;
}

static int match_run(viso_ctx* c, PlainCache* pc, PlainProf& pp, FramePlan& P, int32_t* out_match, int* out_n, double* tt) {
    hipStream_t s = c->stream; int r;
    if ((r = frame_open(c, pc, P)) < 0 || (r = frame_fill_head(c, pc, P)) < 0 || (r = frame_copy_outs(c, pc, P)) < 0) return r;
    if ((r = plain_blit(s, P.H, P.f->dev, (P.f->o_misc + sizeof(FrameMisc)) / 4)) < 0) return r;
    pp.mark(1);
    if (g_tr_on) tt[3] = tr_now();
    if ((r = frame_queue_first(c, pc, P)) < 0) return r;
    pp.mark(2);
    if (!P.spec_B) {   // no join kernel for the first copy-out to ride in
        hipLaunchKernelGGL(plain_out_kernel, dim3((unsigned)(P.H->outA.n_regions * P.H->outA.gx)), dim3(256), 0, s, P.H->outA);
        HIP_TRY(hipGetLastError());
    }
    pp.mark(3);
    if (P.spec_B && (r = frame_queue_second(c, pc, P)) < 0) return r;
    if (g_tr_on) tt[4] = tr_now();
    pp.wait_begin();
    if ((r = plain_signal_wait(c, s, P.seqA)) < 0) return r;   // the first copy-out: whatever was launched behind it runs on
    pp.wait_end();
    if (g_tr_on) tt[5] = tr_now();
    return frame_harvest(c, pc, P, out_match, out_n);
}

static int match_desc_locked(viso_ctx* c, PlainCache* pc, PlainProf& pp, const float* kp1, int n1, const float* kp2, int n2, const float* d1,
                             const float* d2, int dlen, const viso_match_params* mp, int32_t* out_match, int* out_n) {
    hipStream_t s = c->stream;
    int r;
    const int variant = matcher_effective(c->matcher_variant, dlen), extras = pack_extras(c->matcher_variant, dlen);
    // the planes' shift (matcher variant 6): one call, no previous run to learn it from: the default, or the forced one
    const int r8s = c->row8_force >= 0 ? c->row8_force : VISO_R8_DEFAULT;
    // ---- the two images: resident already, or uploaded now (the uploads start before anything else is prepared)
    if (g_tr_on < 0) { const char* e = getenv("VISO_PLAIN_TRACE"); g_tr_on = e && *e == '1'; }
    double tt[7] = {g_tr_on ? tr_now() : 0, 0, 0, 0, 0, 0, 0};
    int iq = plain_lookup(pc, kp1, d1, n1, dlen, extras, r8s);
    int it = plain_lookup(pc, kp2, d2, n2, dlen, extras, r8s);
    const bool hit_q = iq >= 0, hit_t = it >= 0;
    const bool same_image = !hit_q && !hit_t && kp1 == kp2 && d1 == d2 && n1 == n2;   // one upload serves both sides
    {
        KpImport imp[2];
        int n_imp = 0, cap_imp = 1;
        if (!hit_q) {
            if ((iq = plain_prepare(c, pc, kp1, n1, dlen, extras, r8s, it, -1, &imp[n_imp])) < 0) return iq;
            ++n_imp; cap_imp = n1 > cap_imp ? n1 : cap_imp;
        }
        if (same_image) it = iq;
        else if (!hit_t) {
            if ((it = plain_prepare(c, pc, kp2, n2, dlen, extras, r8s, iq, -1, &imp[n_imp])) < 0) return it;
            ++n_imp; cap_imp = n2 > cap_imp ? n2 : cap_imp;
        }
        // the new images' keypoints: ONE launch, a workgroup per image, while the host copies the rows
        if (n_imp && (r = launch_sort_kp(s, nullptr, n_imp, cap_imp, nullptr, 0, nullptr, imp, n_imp)) < 0) return r;
    }
    if (g_tr_on > 0) { g_tr.acq_us[2] += tr_now() - tt[0]; g_tr.acq_calls += 1; }
    if (!hit_q && (r = plain_finish(c, pc, iq, d1, s)) < 0) return r;
    if (g_tr_on) tt[1] = tr_now();
    if (!hit_t && !same_image && (r = plain_finish(c, pc, it, d2, s)) < 0) return r;
    if (g_tr_on) tt[2] = tr_now();
    const bool stereo_call = mp->enforce_epipolar != 0;
    // ---- a temporal call the frame's stereo call has already answered?
    if (!stereo_call) {
        PlainFrame& cur = pc->frame[pc->cur];
        PlainFrame& prv = pc->frame[pc->cur ^ 1];
        if (pc->speculate && cur.valid)
            for (int p = 1; p < PF_PROBS; ++p)
                if (cur.have[p] && cur.tq[p] == iq && cur.tt[p] == it && pc->slot[iq].stamp == cur.stq[p] &&
                    pc->slot[it].stamp == cur.stt[p] && params_equal(*mp, cur.mp[p])) {
                    const int m = cur.m[p];
                    if (m > 0) memcpy(out_match, frame_rows(cur, p), sizeof(int) * 3 * (size_t)m);
                    *out_n = m;
                    cur.used[p] = true;
                    pc->spec_served[0] += 1;
                    if (g_tr_on > 0) { g_tr.srv_us[0] += tt[2] - tt[0]; g_tr.srv_us[1] += tr_now() - tt[2]; g_tr.srv_n += 1; }
                    return VISO_OK;
                }
        // the direct path it is; remember what a temporal call looks like, and whether it is the loop's
        pc->tm = *mp; pc->tm_known = true;
        if (cur.valid && prv.valid && ((iq == cur.L && it == prv.L && pc->slot[it].stamp == prv.sL) ||
                                       (iq == cur.R && it == prv.R && pc->slot[it].stamp == prv.sR))) pc->tm_pattern = true;
    }
    FramePlan P{};
    P.iq = iq; P.it = it; P.n1 = n1; P.dlen = dlen; P.variant = variant; P.extras = extras; P.r8s = r8s; P.mp = mp; P.stereo = stereo_call;
    for (int pass = 0; pass < 2; ++pass) {   // second pass: the first lacked a kernel that turned out to have work (frame_repeat)
        P.force_general = pass == 1;
        r = match_run(c, pc, pp, P, out_match, out_n, tt);
        if (r != PLAIN_RERUN) break;
    }
    if (r < 0) return r;
    if (g_tr_on) {
        tt[6] = tr_now();
        const int k = (hit_q ? 0 : 1) + (hit_t ? 0 : 1);
        for (int j = 0; j < 6; ++j) g_tr.us[k][j] += tt[j + 1] - tt[j];
        g_tr.n[k] += 1;
    }
    return VISO_OK;
}

// match_desc, reference src/viso.cpp:669-726.
extern "C" int viso_match_desc(const float* kp1, int n1, const float* kp2, int n2, const float* d1, const float* d2, int dlen,
                               const viso_match_params* mp, int32_t* out_match, int* out_n) {
    if (n1 < 0 || n2 < 0 || dlen <= 0 || !mp || !out_n || mp->max_neighbors <= 0 ||
        (n1 && (!kp1 || !d1 || !out_match)) || (n2 && (!kp2 || !d2))) {
        viso_set_error("viso_match_desc: bad argument (the reference asserts d1.cols==d2.cols, src/viso.cpp:676)");
        return VISO_ERR_ARG;
    }
    *out_n = 0;
    if (n1 == 0) return VISO_OK;
    if (n1 > VISO_SORT_MAX || n2 > VISO_SORT_MAX) {
        viso_set_error("viso_match_desc: more than %d keypoints per image is not supported by this build", VISO_SORT_MAX);
        return VISO_ERR_UNSUPPORTED;
    }
    PlainCall call;   // the lock, the context and the profile; the frame machinery below queues and waits by itself
    VISO_TRY(call.begin(VISO_PLAIN_MATCH_DESC));
    PlainCache* pc = plain_cache(call.c);
    if (!pc) { viso_set_error("viso_match_desc: out of memory"); return VISO_ERR_NOMEM; }
    const int r = match_desc_locked(call.c, pc, call.pp, kp1, n1, kp2, n2, d1, d2, dlen, mp, out_match, out_n);
    if (r < 0) plain_quiesce(call.c, pc);
    return r;
}

// ---- the frame's other calls (circle.hip asks before it goes to the device) ----------------------------------------
// collect_matches(kp1, kp2, match) of the stereo call's own output: x is there already.  1 = served, 0 = not.
int plain_try_collect(viso_ctx* c, const float* kp1, int n1, const float* kp2, int n2, const int32_t* match, int n, double* x) {
    PlainCache* pc = c->plain;
    if (!pc || !pc->speculate) return 0;
    PlainFrame& f = pc->frame[pc->cur];
    if (!f.valid || !f.have[0] || f.m[0] != n || n <= 0) return 0;
    const PlainSlot &a = pc->slot[f.L], &b = pc->slot[f.R];
    if (!a.valid || !b.valid || a.stamp != f.sL || b.stamp != f.sR || a.n != n1 || b.n != n2) return 0;
    if (memcmp(a.pin, kp1, sizeof(float2) * (size_t)n1) != 0 || memcmp(b.pin, kp2, sizeof(float2) * (size_t)n2) != 0) return 0;
    if (memcmp(frame_rows(f, 0), match, sizeof(int) * 3 * (size_t)n) != 0) return 0;
    // the call is the loop's: worth computing ahead from the next frame on
    pc->x_pattern = true;
    if (!f.have_xX) return 0;
    const size_t C = frame_ld(f);
    const double* hx = frame_host<const double>(f, f.o_x);
    for (int k = 0; k < 4; ++k) memcpy(x + (size_t)k * n, hx + C * k, sizeof(double) * (size_t)n);
    f.used_x = true;
    pc->spec_served[1] += 1;
    return 1;
}

// triangulate_rectified(x, param) of that x with the parameters of the last call: X is there already.
int plain_try_triangulate(viso_ctx* c, const double* x, int m, const viso_param* p, double* X) {
    PlainCache* pc = c->plain;
    if (!pc) return 0;
    pc->tri_p = *p; pc->tri_known = true;
    if (!pc->speculate) return 0;
    PlainFrame& f = pc->frame[pc->cur];
    if (!f.valid || !f.have_xX || f.m[0] != m || m <= 0 || !tri_equal(*p, f.tri_p)) return 0;
    const size_t C = frame_ld(f);
    const double* hx = frame_host<const double>(f, f.o_x);
    for (int k = 0; k < 4; ++k)
        if (memcmp(hx + C * k, x + (size_t)k * m, sizeof(double) * (size_t)m) != 0) return 0;
    const double* hX = frame_host<const double>(f, f.o_X);
    for (int k = 0; k < 3; ++k) memcpy(X + (size_t)k * m, hX + C * k, sizeof(double) * (size_t)m);
    f.used_X = true;
    pc->spec_served[2] += 1;
    return 1;
}

static bool rows_equal(const int* a, const int32_t* b, int n) { return n == 0 || memcmp(a, b, sizeof(int) * 3 * (size_t)n) == 0; }

// match_circle(match_lr, match_lr_prev, match11, match22) of the frame's own four lists: joined already.
int plain_try_circle(viso_ctx* c, const int32_t* lr, int n_lr, const int32_t* lr_prev, int n_lrp, const int32_t* m11, int n11,
                     const int32_t* m22, int n22, int32_t* circ, int32_t* pcl, int cap, int* out_n, int* ret) {
    PlainCache* pc = c->plain;
    if (!pc || !pc->speculate) return 0;
    PlainFrame& f = pc->frame[pc->cur];
    PlainFrame& prv = pc->frame[pc->cur ^ 1];
    if (!f.valid || !prv.valid || !f.have[0] || !prv.have[0] || f.m[0] != n_lr || prv.m[0] != n_lrp) return 0;
    if (!rows_equal(frame_rows(f, 0), lr, n_lr) || !rows_equal(frame_rows(prv, 0), lr_prev, n_lrp)) return 0;
    const bool full = f.have[1] && f.have[2] && f.m[1] == n11 && f.m[2] == n22 && rows_equal(frame_rows(f, 1), m11, n11) && rows_equal(frame_rows(f, 2), m22, n22);
    if (f.have[1] && f.have[2] && !full) return 0;
    pc->circ_pattern = true;   // the loop's call: the stereo lists of this frame and the last
    if (!f.have_B || !full) return 0;
    if (frame_wait(c, f, 0) < 0) return 0;
    const int cnt = f.n_circ;
    if (cnt < 0 || cnt > f.cap) return 0;
    const int w = cnt < cap ? cnt : cap;
    const int* rows = frame_host<const int>(f, f.o_circ);
    for (int i = 0; i < w; ++i) {
        circ[4 * i + 0] = rows[6 * i + 0]; circ[4 * i + 1] = rows[6 * i + 1]; circ[4 * i + 2] = rows[6 * i + 2]; circ[4 * i + 3] = rows[6 * i + 3];
        pcl[2 * i + 0] = rows[6 * i + 4]; pcl[2 * i + 1] = rows[6 * i + 5];
    }
    *out_n = cnt;
    f.used_circ = true;
    pc->circ_seen_no = pc->frame_no; pc->circ_seen_cnt = cnt;
    pc->spec_served[2] += 1;
    *ret = VISO_OK;
    if (cnt > cap) { viso_set_error("viso_match_circle: %d rows needed, cap %d", cnt, cap); *ret = VISO_ERR_ARG; }
    return 1;
}

// match_circle took the direct path with `cnt` rows: remember it (the RANSAC call of the same frame is recognised by it)
void plain_note_circle(viso_ctx* c, int cnt) {
    PlainCache* pc = c->plain;
    if (!pc) return;
    pc->circ_seen_no = pc->frame_no; pc->circ_seen_cnt = cnt;
}

static bool rs_param_equal(const viso_param& a, const viso_param& b) {   // every field the solver reads, bit for bit
    return tri_equal(a, b) && a.ransac_iter == b.ransac_iter && memcmp(&a.inlier_threshold, &b.inlier_threshold, 8) == 0 &&
           memcmp(&a.thresh, &b.thresh, 8) == 0;
}

// ransac_minimize_reproj on the gathered columns of that join, with the parameters and the stream key that were expected.
int plain_try_ransac(viso_ctx* c, const double* X, const double* obs, int m, double best_tr[6], int32_t* best_inl, int* n_inl,
                     const viso_param* p, const int32_t* samples, uint64_t seed, uint64_t frame, int* ret) {
    PlainCache* pc = c->plain;
    if (!pc) return 0;
    PlainFrame& f = pc->frame[pc->cur];
    bool served = false;
    if (pc->speculate && !samples && f.valid && f.have_B && rs_param_equal(*p, f.rs_p) && seed == f.rs_seed && frame == f.rs_frame &&
        frame_wait(c, f, 1) >= 0 && f.n_circ == m && m >= 3 && m <= f.cap) {
        const size_t C = frame_ld(f);
        const double* hXp = frame_host<const double>(f, f.o_Xpc);
        const double* hxc = frame_host<const double>(f, f.o_xc);
        bool same = true;
        for (int k = 0; k < 3 && same; ++k) same = memcmp(hXp + C * k, X + (size_t)k * m, sizeof(double) * (size_t)m) == 0;
        for (int k = 0; k < 4 && same; ++k) same = memcmp(hxc + C * k, obs + (size_t)k * m, sizeof(double) * (size_t)m) == 0;
        const RansacOut* rso = frame_host<const RansacOut>(f, f.o_rs);
        if (same && rso->n_inl >= 0 && rso->n_inl <= m) {
            // computed ahead without knowing the caller's best_tr: where the reference would leave it alone (no hypothesis with
            // support, src/viso.cpp:1564-1568) the stage wrote none and says so in `kept`
            if (!rso->kept) memcpy(best_tr, rso->tr, sizeof(double) * 6);
            *n_inl = rso->n_inl;
            if (rso->n_inl > 0) memcpy(best_inl, rso->inl, sizeof(int) * (size_t)rso->n_inl);
            *ret = rso->ok ? 1 : 0;
            f.used_rs = true;
            pc->spec_served[3] += 1;
            served = true;
        }
    }
    if (!samples) {   // what the next frame's call is expected to look like
        const uint64_t d = frame - pc->rs_last_frame;
        pc->rs_delta_stable = pc->rs_known && d == pc->rs_delta;
        pc->rs_delta = d; pc->rs_last_frame = frame; pc->rs_seed = seed; pc->rs_p = *p; pc->rs_known = true;
        if (served || (pc->circ_seen_no == pc->frame_no && pc->circ_seen_cnt == m)) pc->rs_pattern = true;
    }
    return served ? 1 : 0;
}
