// batch.hip — device-resident frame batches: the loop body of
// sequence_odometry (reference src/viso.cpp:1205-1327) for many frames per
// launch, every stage on one HIP stream with no host round trip in between.
// struct viso_batch, the HBM layout and the map of the three batch files are in batch.h.  Here: the batch's life, its uploads, the
// run itself and the core getters; the opt-in stages that belong to the uploads and the matcher (rectify, sub-pixel) with them.
#include "batch.h"

#include <algorithm>

void viso_batch::own(void** p) {
    if (std::find(owned.begin(), owned.end(), p) == owned.end()) owned.push_back(p);
}

int viso_batch::alloc_bytes(void** p, size_t bytes) {
    *p = nullptr;
    HIP_TRY(hipMalloc(p, bytes ? bytes : 1));
    own(p);
    return VISO_OK;
}

int viso_batch::alloc_zeroed(std::initializer_list<DBuf> bufs) {
    int r = VISO_OK;
    for (const DBuf& d : bufs) *d.p = nullptr;
    for (const DBuf& d : bufs)
        if ((r = alloc_bytes(d.p, d.bytes)) < 0) break;
    if (r < 0) {
        for (const DBuf& d : bufs) (void)release_bytes(d.p);
        return r;
    }
    for (const DBuf& d : bufs) HIP_TRY(hipMemset(*d.p, 0, d.bytes));
    return VISO_OK;
}

int viso_batch::release_bytes(void** p) {   // the pointer stays recorded: null until the next allocation fills it
    void* q = *p;
    *p = nullptr;
    if (q) HIP_TRY(hipFree(q));
    return VISO_OK;
}

int viso_batch::fit_bytes(void** p, size_t* have, size_t want, bool grow_only, const char* where, const char* what) {
    if (*p && (grow_only ? *have >= want : *have == want)) return VISO_OK;
    if (*p) VISO_TRY(batch_sync(this));
    *have = 0;
    VISO_TRY(release_bytes(p));
    const hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        if (what) { viso_set_error("%s: cannot allocate the %zu-byte %s", where, want, what); return VISO_ERR_NOMEM; }
        viso_set_error("hipMalloc(%zu) -> %s", want, hipGetErrorString(e));
        return VISO_ERR_HIP;
    }
    own(p);
    *have = want;
    return VISO_OK;
}

// Frees everything it can; the first HIP error met is recorded (viso_last_error) and returned.  Like
// viso_ctx_destroy it must run before the HIP runtime starts unloading (not from static destructors).
extern "C" int viso_batch_destroy(viso_batch* b) {
    if (!b) return VISO_OK;
    // the registry decides: a live handle is ours to free; one that viso_ctx_destroy of its context already freed is a no-op
    // (the context left a tombstone for it); anything else -- a second destroy, a pointer that never was a batch -- is an
    // argument error, never a dereference
    const int st = viso_batch_unregister(b);
    if (st == 0) { delete b; return VISO_OK; }   // the shell its context left behind (viso_batch_free(b, true)): nothing else to free
    if (st < 0) { viso_set_error("viso_batch_destroy: not a live batch handle"); return VISO_ERR_ARG; }
    return viso_batch_free(b, false);
}

// Frees a batch that has left the registry (viso_batch_destroy, or viso_ctx_destroy for the batches still alive on it).
// keep_shell (viso_ctx_destroy): everything the batch owns goes, the small host object itself stays allocated until the caller's
// own viso_batch_destroy -- a freed address could be handed to ANOTHER batch (of another thread) meanwhile, and the late
// destroy this library promises to tolerate would then hit that one.
int viso_batch_free(viso_batch* b, bool keep_shell) {
    hipError_t first = hipSuccess;
    auto note = [&](hipError_t e) { if (e != hipSuccess && first == hipSuccess) first = e; };
    note(hipSetDevice(b->ctx->device));
    note(hipStreamSynchronize(b->ctx->stream));
    if (b->solver_stream) note(hipStreamSynchronize(b->solver_stream));   // the context's: not destroyed here
    if (b->ev_join) note(hipEventDestroy(b->ev_join));
    if (b->ev_ransac) note(hipEventDestroy(b->ev_ransac));
    for (int k = 0; k < 3; ++k) if (b->ev_stamp[k]) note(hipEventDestroy(b->ev_stamp[k]));
    for (auto& e : b->events) { note(hipEventDestroy(e.first)); note(hipEventDestroy(e.second)); }
    for (int k = 0; k < VISO_NPIN_SLOTS; ++k) if (b->n_pin_ev[k]) note(hipEventDestroy(b->n_pin_ev[k]));
    if (b->n_pin) note(hipHostFree(b->n_pin));
    if (b->r8pin) note(hipHostFree(b->r8pin));
    if (b->pose_pin) note(hipHostFree(b->pose_pin));
    if (b->r8ev) note(hipEventDestroy(b->r8ev));
    for (void** p : b->owned) if (*p) { note(hipFree(*p)); *p = nullptr; }
    if (keep_shell) {   // the shell owns nothing, heap included
        b->ctx = nullptr;
        b->events.clear(); b->events.shrink_to_fit();
        b->desc_family.clear(); b->desc_family.shrink_to_fit();
        b->owned.clear(); b->owned.shrink_to_fit();
    }
    else delete b;
    if (first != hipSuccess) { viso_set_error("viso_batch_destroy: %s", hipGetErrorString(first)); return VISO_ERR_HIP; }
    return VISO_OK;
}

static int build_items(viso_batch* b) {
    const int nf = b->nf, cap = b->cap;
    const size_t kpi = (size_t)cap, dsi = (size_t)cap * VISO_ROW, dfi = (size_t)cap * b->dlen;
    // image views: index t*2+side, plus one empty view (n -> 0) for padding problems
    std::vector<ImageView> V((size_t)nf * 2 + 1);
    for (int t = 0; t < nf; ++t)
        for (int side = 0; side < 2; ++side) {
            const size_t i = (size_t)t * 2 + side;
            ImageView& v = V[i];
            v.kp = b->kp + i * kpi; v.frows = b->desc + i * dfi; v.n = b->n + i;
            v.skp = b->skp + i * kpi; v.sidx = b->sidx + i * kpi; v.rank = b->rank + i * kpi;
            v.bstart = b->bstart + i * (VISO_NB + 1); v.xinfo = b->xinfo + i * 8;
            v.rows = b->packed + i * dsi;
            v.sums = b->sums + i * kpi;
            v.rows8 = b->packed8 + i * kpi * VISO_ROW8;
            v.qord = b->qord + i * (((size_t)cap + 63) & ~(size_t)63);
            v.bad = b->bad_img + i;
        }
    {
        ImageView& e = V[(size_t)nf * 2];
        e = V[0];
        e.n = b->zero;
        e.bad = b->zero + 5;
    }
    HIP_TRY(hipMemcpy(b->views, V.data(), sizeof(ImageView) * V.size(), hipMemcpyHostToDevice));
    std::vector<MatchProblem> P((size_t)b->n_probs);
    for (auto& p : P) { memset(&p, 0, sizeof(p)); p.tile_flag = b->tile_flag; p.q = V[(size_t)nf * 2]; p.t = V[(size_t)nf * 2]; p.m_cnt = b->zero + 1; p.scored = (unsigned long long*)(b->zero + 2); p.ovf = b->ovf_q; p.ovf_cnt = b->ovf_cnt; p.res = b->res; p.sorted = b->sorted; p.pos = b->pos; }
    auto img_kp = [&](int t, int side) { return b->kp + ((size_t)t * 2 + side) * kpi; };
    for (int t = 0; t < nf; ++t) {
        for (int which = 0; which < 3; ++which) {
            if (which > 0 && t == 0) continue;   // first frame has no predecessor (:1256-1260)
            MatchProblem& p = P[(size_t)prob_slot(which, t)];
            int qs, qt, ts, tt;                  // query side/frame, target side/frame
            if (which == 0) { qs = 0; qt = t; ts = 1; tt = t; }          // match_desc(kp1,kp2,...) :1240
            else if (which == 1) { qs = 0; qt = t; ts = 0; tt = t - 1; } // (kp1,kp1_prev) :1264
            else { qs = 1; qt = t; ts = 1; tt = t - 1; }                 // (kp2,kp2_prev) :1275
            p.q = V[(size_t)qt * 2 + qs];
            p.t = V[(size_t)tt * 2 + ts];
            const size_t o = (size_t)which * nf + t;
            p.res = b->res + o * cap; p.sorted = b->sorted + o * cap * 3; p.pos = b->pos + o * cap;
            p.m_cnt = b->m_cnt + o; p.scored = b->scored + o;
            p.ovf = b->ovf_q; p.ovf_cnt = b->ovf_cnt;   // one queue and one counter for the whole launch
            p.tile_flag = b->tile_flag + o * b->tiles;
            p.pidx = which == 0 ? 0 : 1; p.cap = cap;
        }
    }
    HIP_TRY(hipMemcpy(b->probs, P.data(), sizeof(MatchProblem) * P.size(), hipMemcpyHostToDevice));
    if (nf > 1) {
        std::vector<JoinItem> J((size_t)nf - 1);
        for (int t = 1; t < nf; ++t) {
            JoinItem& j = J[(size_t)t - 1];
            j.lr = b->sorted + ((size_t)0 * nf + t) * cap * 3; j.lr_cnt = b->m_cnt + t;
            j.res11 = b->res + ((size_t)1 * nf + t) * cap;
            j.res22 = b->res + ((size_t)2 * nf + t) * cap;
            j.pos_lrp = b->pos + ((size_t)0 * nf + (t - 1)) * cap;
            j.res_lrp = b->res + ((size_t)0 * nf + (t - 1)) * cap;
            j.kp1 = img_kp(t, 0); j.kp2 = img_kp(t, 1); j.kp1p = img_kp(t - 1, 0); j.kp2p = img_kp(t - 1, 1);
            j.circ = b->circ + (size_t)t * cap * 4; j.pcl = b->pcl + (size_t)t * cap * 2; j.mc = b->mc + t;
            j.x_c = b->x_c + (size_t)t * 4 * cap; j.Xp_c = b->Xp_c + (size_t)t * 3 * cap; j.ldc = cap;
            j.uv = b->uv ? b->uv + (size_t)t * cap : nullptr; j.uvp = b->uv ? b->uv + (size_t)(t - 1) * cap : nullptr;
        }
        HIP_TRY(hipMemcpy(b->join, J.data(), sizeof(JoinItem) * J.size(), hipMemcpyHostToDevice));
    }
    return VISO_OK;
}

static int build_solver_items(viso_batch* b) {
    const int nf = b->nf, cap = b->cap, iters = b->iters;
    if (nf <= 1) return VISO_OK;
    std::vector<SolverItem> S((size_t)nf - 1);
    for (int t = 1; t < nf; ++t) {
        SolverItem& s = S[(size_t)t - 1];
        memset(&s, 0, sizeof(s));
        s.X = b->Xp_c + (size_t)t * 3 * cap; s.obs = b->x_c + (size_t)t * 4 * cap;
        s.m_ptr = b->mc + t; s.ld = cap; s.samples = nullptr; s.samp_h = b->samp_h + (size_t)t * iters * 3;
        s.frame = b->first_frame + (unsigned long long)t;
        s.tr_h = b->tr_h + (size_t)t * iters * 6; s.ok_h = b->ok_h + (size_t)t * iters; s.cnt_h = b->cnt_h + (size_t)t * iters;
        s.rot = b->rot + (size_t)t * viso_rot_bytes(iters);
        s.tr = b->tr + (size_t)t * 6; s.ok = b->ok + t; s.n_inl = b->n_inl + t; s.inl = b->inl + (size_t)t * cap;
    }
    HIP_TRY(hipMemcpy(b->sitems, S.data(), sizeof(SolverItem) * S.size(), hipMemcpyHostToDevice));
    return VISO_OK;
}

// Everything viso_batch_create allocates (events, pinned mirrors, device buffers) and the buffers' first contents.  On an error the
// caller frees what exists so far.
static int create_buffers(viso_batch* b) {
    const size_t nf = (size_t)b->nf, c = (size_t)b->cap;
    if (b->ctx->solver_stream) {
        if (hipEventCreateWithFlags(&b->ev_join, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&b->ev_ransac, hipEventDisableTiming) != hipSuccess) {
            viso_set_error("viso_batch_create: event creation failed");
            return VISO_ERR_HIP;
        }
        b->solver_stream = b->ctx->solver_stream;
    }
    VISO_TRY(b->alloc(&b->kp, nf * 2 * c)); VISO_TRY(b->alloc(&b->desc, nf * 2 * c * b->dlen)); VISO_TRY(b->alloc(&b->n, nf * 2));
    VISO_TRY(b->alloc(&b->packed, nf * 2 * c * VISO_ROW)); VISO_TRY(b->alloc(&b->packed8, nf * 2 * c * VISO_ROW8));
    VISO_TRY(b->alloc(&b->r8cnt, 4)); VISO_TRY(b->alloc(&b->sums, nf * 2 * c)); VISO_TRY(b->alloc(&b->zero, 8));
    VISO_TRY(b->alloc(&b->probs, (size_t)b->n_probs));
    VISO_TRY(b->alloc(&b->skp, nf * 2 * c)); VISO_TRY(b->alloc(&b->sidx, nf * 2 * c)); VISO_TRY(b->alloc(&b->rank, nf * 2 * c));
    VISO_TRY(b->alloc(&b->bstart, nf * 2 * (VISO_NB + 1))); VISO_TRY(b->alloc(&b->xinfo, nf * 2 * 8)); VISO_TRY(b->alloc(&b->views, nf * 2 + 1));
    VISO_TRY(b->alloc(&b->qord, nf * 2 * ((c + 63) & ~(size_t)63)));
    VISO_TRY(b->alloc(&b->res, 3 * nf * c)); VISO_TRY(b->alloc(&b->sorted, 3 * nf * c * 3)); VISO_TRY(b->alloc(&b->pos, 3 * nf * c));
    VISO_TRY(b->alloc(&b->m_cnt, 3 * nf));
    VISO_TRY(b->alloc(&b->ovf_q, 3 * nf * c));
    b->tiles = (b->cap + 63) / 64;
    VISO_TRY(b->alloc(&b->tile_flag, 3 * nf * (size_t)b->tiles));
    // per-run counters zeroed by ONE memset: scored[3nf] (u64) | ovf_cnt[3nf] (int) | bad_img[2nf] (int) | bad_any (int)
    b->zeroed_bytes = 3 * nf * sizeof(unsigned long long) + (3 * nf + 2 * nf + 4) * sizeof(int);
    VISO_TRY(b->alloc(&b->scored, b->zeroed_bytes / sizeof(unsigned long long) + 1));
    b->ovf_cnt = reinterpret_cast<int*>(b->scored + 3 * nf);
    b->bad_img = b->ovf_cnt + 3 * nf;
    b->bad_any = b->bad_img + 2 * nf;
    VISO_TRY(b->alloc(&b->x_c, nf * 4 * c)); VISO_TRY(b->alloc(&b->Xp_c, nf * 3 * c));
    VISO_TRY(b->alloc(&b->join, nf)); VISO_TRY(b->alloc(&b->sitems, nf));
    VISO_TRY(b->alloc(&b->circ, nf * c * 4)); VISO_TRY(b->alloc(&b->pcl, nf * c * 2)); VISO_TRY(b->alloc(&b->mc, nf));
    // poses, flags and inlier counts in one block: one blit into the pinned mirror per run (three blocking copies of a
    // few bytes were 50 us of a one-pair batch's 0.42 ms)
    b->pose_bytes = nf * (6 * sizeof(double) + 2 * sizeof(int));
    VISO_TRY(b->alloc_bytes(reinterpret_cast<void**>(&b->tr), b->pose_bytes));
    b->ok = reinterpret_cast<int*>(b->tr + nf * 6);
    b->n_inl = b->ok + nf;
    VISO_TRY(b->alloc(&b->inl, nf * c));
    if (hipHostMalloc((void**)&b->pose_pin, b->pose_bytes, hipHostMallocDefault) != hipSuccess) {
        b->pose_pin = nullptr;
        viso_set_error("viso_batch_create: hipHostMalloc of the pose mirror failed");
        return VISO_ERR_NOMEM;
    }
    memset(b->pose_pin, 0, b->pose_bytes);
    if (hipHostMalloc((void**)&b->r8pin, sizeof(int) * 4, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&b->r8ev, hipEventDisableTiming) != hipSuccess) {
        viso_set_error("viso_batch_create: pinned buffer / event for the planes' statistics failed");
        return VISO_ERR_HIP;
    }
    if (hipHostMalloc((void**)&b->n_pin, sizeof(int) * VISO_NPIN_SLOTS * 2 * nf, hipHostMallocDefault) != hipSuccess) {
        b->n_pin = nullptr;
        viso_set_error("viso_batch_create: hipHostMalloc of the n staging ring failed");
        return VISO_ERR_NOMEM;
    }
    for (int k = 0; k < VISO_NPIN_SLOTS; ++k)
        if (hipEventCreateWithFlags(&b->n_pin_ev[k], hipEventDisableTiming) != hipSuccess) { b->n_pin_ev[k] = nullptr; return VISO_ERR_HIP; }
    const bool ok = hipMemset(b->zero, 0, 8 * sizeof(int)) == hipSuccess &&
                    hipMemset(b->n, 0, nf * 2 * sizeof(int)) == hipSuccess &&
                    hipMemset(b->m_cnt, 0, 3 * nf * sizeof(int)) == hipSuccess &&
                    hipMemset(b->mc, 0, nf * sizeof(int)) == hipSuccess &&
                    hipMemset(b->tr, 0, b->pose_bytes) == hipSuccess &&
                    hipMemset(b->scored, 0, b->zeroed_bytes) == hipSuccess;
    if (!ok || build_items(b) < 0) { viso_set_error("viso_batch_create: device initialisation failed"); return VISO_ERR_HIP; }
    return VISO_OK;
}

extern "C" viso_batch* viso_batch_create(viso_ctx* ctx, int n_frames, int cap, int dlen) {
    if (!ctx || n_frames <= 0 || cap <= 0 || dlen <= 0) { viso_set_error("viso_batch_create: bad argument"); return nullptr; }
    if (!viso_ctx_live(ctx)) { viso_set_error("viso_batch_create: not a live context handle"); return nullptr; }
    if (hipSetDevice(ctx->device) != hipSuccess) { viso_set_error("hipSetDevice failed"); return nullptr; }
    viso_batch* b = new viso_batch();
    b->ctx = ctx; b->nf = n_frames; b->cap = cap; b->dlen = dlen;
    b->n_probs = ((n_frames + 7) / 8) * 24;
    b->desc_family.assign((size_t)n_frames, 0);
    if (create_buffers(b) < 0) { viso_batch_free(b, false); return nullptr; }
    if (!viso_batch_register(ctx, b)) { viso_set_error("viso_batch_create: the context was destroyed meanwhile"); viso_batch_free(b, false); return nullptr; }
    return b;
}

// The argument checks every upload shares: a live batch, frames f0 .. f0+nf-1 inside it, what else the entry point asks of its
// arguments (rest_ok, which must not read the batch), and the keypoint counts n[2 nf], where given, within the capacity.
static int check_upload(const char* where, viso_batch* b, int f0, int nf, const int32_t* n_or_null, bool rest_ok) {
    if (dead(b) || f0 < 0 || nf < 0 || f0 + nf > b->nf || !rest_ok) { viso_set_error("%s: bad argument", where); return VISO_ERR_ARG; }
    const int32_t* n = n_or_null;
    for (int i = 0; n && i < 2 * nf; ++i)
        if (n[i] < 0 || n[i] > b->cap) { viso_set_error("%s: n[%d]=%d exceeds cap %d", where, i, n[i], b->cap); return VISO_ERR_ARG; }
    return VISO_OK;
}

// Pinned host memory for the *_async uploads (hipHostMalloc): copies from it run as DMA on the context's stream.
extern "C" void* viso_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { viso_set_error("viso_host_alloc: hipHostMalloc(%zu) failed", bytes); return nullptr; }
    return p;
}
extern "C" int viso_host_free(void* p) {
    if (p) HIP_TRY(hipHostFree(p));
    return VISO_OK;
}

// n[2*nf] of the caller -> the next slot of the batch's pinned ring -> device, on stream s.  The caller's array is
// not read after this returns.
static int stage_n_async(viso_batch* b, int f0, int nf, const int32_t* n, hipStream_t s) {
    const int k = b->n_pin_next;
    b->n_pin_next = (k + 1) % VISO_NPIN_SLOTS;
    if (b->n_pin_used[k]) HIP_TRY(hipEventSynchronize(b->n_pin_ev[k]));   // the copy that read this slot VISO_NPIN_SLOTS uploads ago
    int* slot = b->n_pin + (size_t)k * 2 * b->nf;
    memcpy(slot, n, sizeof(int) * (size_t)nf * 2);
    HIP_TRY(hipMemcpyAsync(b->n + (size_t)f0 * 2, slot, sizeof(int) * (size_t)nf * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(b->n_pin_ev[k], s));
    b->n_pin_used[k] = true;
    return VISO_OK;
}

// The body of the four descriptor-in uploads.  The three copies are enqueued on the context's stream (the batch's kernels run on
// that non-blocking stream: behind the batch's previous run, in front of the next one); `n` is validated now and copied through a
// small pinned slot of the batch, so the caller's n array need not be pinned.  sync: wait for the copies.  Without it the host
// buffers must stay untouched until the stream has passed the copies (viso_ctx_synchronize, or any result getter of a later
// run); with buffers from viso_host_alloc the copies are true DMA and overlap the kernels of other contexts.
// esz 2: the descriptors as int16 (N x dlen, tightly packed): the lossless encoding of the reference's Sobel windows (integers
// in [-1020, 1020], src/viso.cpp:1004-1024) at half the bytes of the CV_32F boundary layout.  They live in the same
// device buffer as the f32 rows (reinterpreted), so all frames of a batch must come through ONE of the two families;
// the last upload decides which pack kernel the next run uses.
static int upload_impl(viso_batch* b, int f0, int nf, const float* kp, const void* desc, size_t esz, const int32_t* n, bool sync,
                       const char* who) {
    const bool i16 = esz == sizeof(int16_t);
    VISO_TRY(check_upload(who, b, f0, nf, n, !nf || (kp && desc && n)));
    if (i16 && b->dlen > VISO_ROW) { viso_set_error("%s: int16 descriptors need dlen <= %d", who, VISO_ROW); return VISO_ERR_UNSUPPORTED; }
    if (nf == 0) return VISO_OK;
    VISO_TRY(enter(b));
    b->desc_i16 = i16;
    for (int t = f0; t < f0 + nf; ++t) b->desc_family[(size_t)t] = i16 ? 2 : 1;
    hipStream_t s = b->ctx->stream;
    const size_t c = (size_t)b->cap, row = (size_t)b->dlen * esz;
    HIP_TRY(hipMemcpyAsync(b->kp + (size_t)f0 * 2 * c, kp, sizeof(float2) * (size_t)nf * 2 * c, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(b->desc) + (size_t)f0 * 2 * c * row, desc, (size_t)nf * 2 * c * row, hipMemcpyHostToDevice, s));
    VISO_TRY(stage_n_async(b, f0, nf, n, s));
    if (sync) HIP_TRY(hipStreamSynchronize(s));
    return VISO_OK;
}
extern "C" int viso_batch_upload(viso_batch* b, int f0, int nf, const float* kp, const float* desc, const int32_t* n) {
    return upload_impl(b, f0, nf, kp, desc, sizeof(float), n, true, "viso_batch_upload");
}
extern "C" int viso_batch_upload_async(viso_batch* b, int f0, int nf, const float* kp, const float* desc, const int32_t* n) {
    return upload_impl(b, f0, nf, kp, desc, sizeof(float), n, false, "viso_batch_upload_async");
}
extern "C" int viso_batch_upload_i16(viso_batch* b, int f0, int nf, const float* kp, const int16_t* desc16, const int32_t* n) {
    return upload_impl(b, f0, nf, kp, desc16, sizeof(int16_t), n, true, "viso_batch_upload_i16");
}
extern "C" int viso_batch_upload_i16_async(viso_batch* b, int f0, int nf, const float* kp, const int16_t* desc16, const int32_t* n) {
    return upload_impl(b, f0, nf, kp, desc16, sizeof(int16_t), n, false, "viso_batch_upload_i16_async");
}

// The image buffer for rows x cols images (the caller has synchronised the batch's stream).  The Harris response image of
// viso_batch_detect is sized by the geometry it first met: it goes with the old buffer.
static int ensure_images(viso_batch* b, int rows, int cols) {
    if (b->images && (rows != b->img_rows || cols != b->img_cols)) {
        VISO_TRY(b->release(&b->images));
        VISO_TRY(b->release(&b->h_resp));
        b->dense.last = 0;   // the maps were of the old geometry (their buffer follows at the next disparity launch)
    }
    if (!b->images) {
        VISO_TRY(b->alloc(&b->images, (size_t)rows * cols * 2 * (size_t)b->nf));
        b->img_rows = rows; b->img_cols = cols;
    }
    return VISO_OK;
}

// Rectification on: raw images of frames f0 .. f0+nf-1 -> the staging buffer -> rectify_remap_kernel -> the image buffer, all on s.
// One launch per upload: the maps are read once per upload, not once per frame.
static int upload_raw(viso_batch* b, int f0, int nf, const uint8_t* images, hipStream_t s) {
    const BatchRectify& R = b->rect;
    const StereoImages raw = image_block(R.raw, R.raw_rows, R.raw_cols, f0, nf);
    HIP_TRY(hipMemcpyAsync(raw.img, images, raw.fs * (size_t)nf, hipMemcpyHostToDevice, s));
    return launch_rectify(s, raw, batch_images(b, f0, nf), R.map, R.border);
}

// With rectification on, the images of an upload must be the raw ones.
static int check_raw_geometry(const char* where, viso_batch* b, int rows, int cols) {
    if (!b->rect.map || (rows == b->rect.raw_rows && cols == b->rect.raw_cols)) return VISO_OK;
    viso_set_error("%s: rectification is on: the images must be raw, %d x %d (got %d x %d)", where, b->rect.raw_rows, b->rect.raw_cols, rows, cols);
    return VISO_ERR_ARG;
}

extern "C" int viso_batch_upload_images_async(viso_batch* b, int f0, int nf, const uint8_t* images, int rows, int cols,
                                              const float* kp, const int32_t* n) {
    const char* where = "viso_batch_upload_images_async";
    VISO_TRY(check_upload(where, b, f0, nf, n, rows > 0 && cols > 0 && (!nf || images) && (kp == nullptr) == (n == nullptr)));
    VISO_TRY(check_raw_geometry(where, b, rows, cols));
    if (!b->rect.map && (!b->images || rows != b->img_rows || cols != b->img_cols)) {
        viso_set_error("viso_batch_upload_images_async: image buffers not allocated for %d x %d (call viso_batch_upload_images once first)", rows, cols);
        return VISO_ERR_ARG;
    }
    if (nf == 0) return VISO_OK;
    VISO_TRY(enter(b));
    hipStream_t s = b->ctx->stream;
    const size_t per = (size_t)rows * cols, c = (size_t)b->cap;
    if (b->rect.map) VISO_TRY(upload_raw(b, f0, nf, images, s));
    else HIP_TRY(hipMemcpyAsync(b->images + (size_t)f0 * 2 * per, images, per * 2 * (size_t)nf, hipMemcpyHostToDevice, s));
    if (kp) {
        HIP_TRY(hipMemcpyAsync(b->kp + (size_t)f0 * 2 * c, kp, sizeof(float2) * (size_t)nf * 2 * c, hipMemcpyHostToDevice, s));
        return stage_n_async(b, f0, nf, n, s);
    }
    return VISO_OK;
}

extern "C" int viso_batch_upload_images(viso_batch* b, int f0, int nf, const uint8_t* images, int rows, int cols,
                                        const float* kp, const int32_t* n) {
    const char* where = "viso_batch_upload_images";
    VISO_TRY(check_upload(where, b, f0, nf, n, rows > 0 && cols > 0 && (!nf || images) && (kp == nullptr) == (n == nullptr)));
    VISO_TRY(check_raw_geometry(where, b, rows, cols));
    VISO_TRY(enter(b));
    const size_t c = (size_t)b->cap;
    if (b->rect.map) {   // raw images: staged and rectified on the batch's stream, behind the run in flight
        if (nf == 0) return VISO_OK;
        hipStream_t s = b->ctx->stream;
        VISO_TRY(upload_raw(b, f0, nf, images, s));
        if (kp) {
            HIP_TRY(hipMemcpyAsync(b->kp + (size_t)f0 * 2 * c, kp, sizeof(float2) * (size_t)nf * 2 * c, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(b->n + (size_t)f0 * 2, n, sizeof(int) * (size_t)nf * 2, hipMemcpyHostToDevice, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
        return VISO_OK;
    }
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));   // a run in flight may still read what the (null-stream) copies below rewrite
    VISO_TRY(ensure_images(b, rows, cols));
    const size_t per = (size_t)rows * cols;
    if (nf == 0) return VISO_OK;
    HIP_TRY(hipMemcpy(b->images + (size_t)f0 * 2 * per, images, per * 2 * (size_t)nf, hipMemcpyHostToDevice));
    if (kp) {   // keypoints may instead come from viso_batch_detect
        HIP_TRY(hipMemcpy(b->kp + (size_t)f0 * 2 * c, kp, sizeof(float2) * (size_t)nf * 2 * c, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b->n + (size_t)f0 * 2, n, sizeof(int) * (size_t)nf * 2, hipMemcpyHostToDevice));
    }
    return VISO_OK;
}

// Opt-in rectification of raw images (not in the reference; rectify.hip).  Synchronous like the other setters: the batch's work
// in flight finishes first, then the maps are quantised on the host and the buffers (re)allocated.
extern "C" int viso_batch_set_rectify(viso_batch* b, int raw_rows, int raw_cols, int out_rows, int out_cols, const float* mapxL,
                                      const float* mapyL, const float* mapxR, const float* mapyR, int border) {
    const int given = (mapxL != nullptr) + (mapyL != nullptr) + (mapxR != nullptr) + (mapyR != nullptr);
    if (dead(b) || (given != 0 && given != 4) ||
        (given == 4 && (!rect_geometry_ok(raw_rows, raw_cols, out_rows, out_cols) || border < 0 || border > 255))) {
        viso_set_error("viso_batch_set_rectify: bad argument (sizes > 0, border 0..255, all four maps or none)");
        return VISO_ERR_ARG;
    }
    VISO_TRY(enter(b));
    VISO_TRY(batch_sync(b));
    BatchRectify& R = b->rect;
    VISO_TRY(b->release(&R.map));
    if (given == 0) {   // off: the staging buffer goes too; the image buffer stays (the next upload decides its geometry)
        R.raw_bytes = 0; R.raw_rows = R.raw_cols = 0;
        return b->release(&R.raw);
    }
    const size_t oper = (size_t)out_rows * out_cols;
    std::vector<RectEntry> q(2 * oper);
    rect_quantise(mapxL, mapyL, oper, raw_rows, raw_cols, q.data());
    rect_quantise(mapxR, mapyR, oper, raw_rows, raw_cols, q.data() + oper);
    VISO_TRY(ensure_images(b, out_rows, out_cols));
    VISO_TRY(b->fit(&R.raw, &R.raw_bytes, (size_t)raw_rows * raw_cols * 2 * (size_t)b->nf));
    VISO_TRY(b->alloc(&R.map, 2 * oper));
    if (hipMemcpy(R.map, q.data(), sizeof(RectEntry) * 2 * oper, hipMemcpyHostToDevice) != hipSuccess) {
        (void)b->release(&R.map);
        viso_set_error("viso_batch_set_rectify: copying the maps failed");
        return VISO_ERR_HIP;
    }
    R.raw_rows = raw_rows; R.raw_cols = raw_cols; R.border = border;
    return VISO_OK;
}

// Diagnostics: the shift of the 8-bit planes the last run used (matcher variant 6; see VISO_R8_* in csrc/common.h).
extern "C" int viso_batch_get_row8_shift(viso_batch* b, int* shift) {
    if (dead(b) || !shift) { viso_set_error("viso_batch_get_row8_shift: bad argument"); return VISO_ERR_ARG; }
    *shift = b->r8last;
    return VISO_OK;
}

extern "C" int viso_batch_device_ptrs(viso_batch* b, void** kp, void** desc, void** n) {
    if (dead(b)) return VISO_ERR_ARG;
    if (kp) *kp = b->kp;
    if (desc) *desc = b->desc;
    if (n) *n = b->n;
    return VISO_OK;
}

extern "C" int viso_batch_set_params(viso_batch* b, const viso_match_params* stereo,
                                     const viso_match_params* temporal, const viso_param* p,
                                     uint64_t seed, uint64_t first_frame_index) {
    if (dead(b) || !stereo || !temporal || !p || p->ransac_iter < 0 || stereo->max_neighbors <= 0 || temporal->max_neighbors <= 0) {
        viso_set_error("viso_batch_set_params: bad argument");
        return VISO_ERR_ARG;
    }
    VISO_TRY(enter(b));
    // kernels of a run still in flight read the solver items rewritten below (null-stream copies do not order
    // against the context's non-blocking stream)
    VISO_TRY(batch_sync(b));
    fill_match_params(&b->mp[0], stereo);
    fill_match_params(&b->mp[1], temporal);
    fill_solver_params(&b->sp, p);
    b->seed = seed; b->first_frame = first_frame_index;
    if (p->ransac_iter != b->iters || !b->tr_h) {
        b->iters = p->ransac_iter;
        const size_t k = (size_t)b->nf * (size_t)(b->iters > 0 ? b->iters : 1);
        (void)b->release(&b->tr_h); (void)b->release(&b->ok_h); (void)b->release(&b->cnt_h);
        (void)b->release(&b->hq); (void)b->release(&b->samp_h); (void)b->release(&b->rot);
        VISO_TRY(b->alloc(&b->tr_h, k * 6)); VISO_TRY(b->alloc(&b->ok_h, k)); VISO_TRY(b->alloc(&b->cnt_h, k));
        VISO_TRY(b->alloc(&b->hq, k + 2)); VISO_TRY(b->alloc(&b->samp_h, k * 3));
        VISO_TRY(b->alloc(&b->rot, (size_t)b->nf * viso_rot_bytes(b->iters)));
        // frame 0 has no solve: its rows are never written, and viso_batch_get_hypotheses hands them out with the rest
        HIP_TRY(hipMemset(b->tr_h, 0, sizeof(double) * 6 * k));
        HIP_TRY(hipMemset(b->ok_h, 0, sizeof(int) * k));
        HIP_TRY(hipMemset(b->cnt_h, 0, sizeof(int) * k));
        HIP_TRY(hipMemset(b->hq, 0, sizeof(int) * 2));   // the list of undecided hypotheses starts empty; every chain leaves it empty
    }
    VISO_TRY(build_solver_items(b));
    b->params_set = true;
    return VISO_OK;
}

extern "C" int viso_batch_kernel_timing(viso_batch* b, int enable) {
    if (dead(b)) return VISO_ERR_ARG;
    b->timing = enable != 0;
    return VISO_OK;
}

// What a run refuses before anything is launched.  Where the dense maps are on, dense_preflight follows (viso_batch_run_images).
static int run_matcher_check(viso_batch* b, bool from_images) {
    if (!dead(b)) b->est.cov.last = b->est.ref.last = b->est.win.last = 0;   // the records of an earlier run are not this run's
    if (dead(b) || !b->params_set) { viso_set_error("viso_batch_run: parameters not set"); return VISO_ERR_ARG; }
    if (from_images && (!b->images || b->dlen != VISO_DESC_LEN)) {
        viso_set_error("viso_batch_run_images: no images uploaded (or descriptor length is not 121)");
        return VISO_ERR_ARG;
    }
    if (from_images) return VISO_OK;
    if (b->dense.on()) {
        viso_set_error("viso_batch_run: dense disparity (viso_batch_set_disparity, viso_batch_set_sgm) needs the images: use viso_batch_run_images, "
                       "or turn it off for descriptor-in runs");
        return VISO_ERR_ARG;
    }
    if (b->subpix) {
        viso_set_error("viso_batch_run: sub-pixel refinement (viso_batch_set_subpixel %d) needs the images: use viso_batch_run_images, "
                       "or set mode 0 for descriptor-in runs", b->subpix);
        return VISO_ERR_ARG;
    }
    // f32 rows and int16 rows share one device buffer: a run over frames of both families would reinterpret one of them (garbage
    // matches, no error) -- refuse it
    bool f32 = false, i16 = false;
    for (signed char f : b->desc_family) { f32 = f32 || f == 1; i16 = i16 || f == 2; }
    if (f32 && i16) {
        viso_set_error("viso_batch_run: frames of this batch were uploaded through both viso_batch_upload (f32 rows) and "
                       "viso_batch_upload_i16 (int16 rows); upload all frames through one family");
        return VISO_ERR_ARG;
    }
    return VISO_OK;
}

static int run_matcher_launch(viso_batch* b, bool from_images) {
    VISO_TRY(enter(b));
    hipStream_t s = b->ctx->stream;
    const int with_sums = pack_extras(b->ctx->matcher_variant, b->dlen);   // block sums / 8-bit planes: what the selected temporal kernel reads
    // the run's counters (scored, ovf_cnt, bad_img, bad_any) are zeroed by the first kernel of the run, not by a memset
    // the shift of this run's 8-bit planes (variant 6): forced, or the smallest that clamps at most one element pair in 256
    // of the sample the last counting run took (frames of a sequence look alike; a resident batch sees its own data
    // again).  Counting runs: the first, then every VISO_R8_EVERY-th; their counts come back asynchronously (no wait: a
    // copy that has not landed yet is looked at by a later run).  Any shift gives the same results: this is speed only
    int* r8cnt = nullptr;
    if (with_sums & VISO_PACK_ROWS8) {
        if (b->r8pending && hipEventQuery(b->r8ev) == hipSuccess) {
            b->r8pending = false;
            const unsigned long long rows = (unsigned)b->r8pin[VISO_R8_ROWS], lim = rows * 64ull / 256ull;
            if (rows) b->r8shift = (unsigned)b->r8pin[VISO_R8_C128] <= lim ? 0 : (unsigned)b->r8pin[VISO_R8_C128 + 1] <= lim ? 1 : (unsigned)b->r8pin[VISO_R8_C128 + 2] <= lim ? 2 : 3;
        }
        if (!b->r8pending && b->ctx->row8_force < 0 && b->r8runs % VISO_R8_EVERY == 0) r8cnt = b->r8cnt;
        ++b->r8runs;
        b->r8last = b->ctx->row8_force >= 0 ? b->ctx->row8_force : b->r8shift;
    }
    const int r8s = b->r8last;
    VISO_TRY(launch_sort_kp(s, b->views, b->nf * 2, b->cap, reinterpret_cast<uint32_t*>(b->scored), (int)(b->zeroed_bytes / 4), r8cnt));
    if (from_images)   // Sobel windows straight into packed rows (never bad: integers in [-1020,1020])
        VISO_TRY(launch_extract_pack(s, b->views, b->cap, batch_images(b, 0, b->nf), with_sums, r8s, r8cnt));
    else if (b->desc_i16)
        VISO_TRY(launch_pack_i16(s, b->views, b->nf * 2, b->cap, b->dlen, reinterpret_cast<const int16_t*>(b->desc), with_sums, r8s, r8cnt));
    else
        VISO_TRY(launch_pack(s, b->views, b->nf * 2, b->cap, b->dlen, b->bad_img, b->bad_any, with_sums, r8s, r8cnt));
    if (r8cnt) {   // the sample's counts on their way to the host
        HIP_TRY(hipMemcpyAsync(b->r8pin, b->r8cnt, sizeof(int) * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(b->r8ev, s));
        b->r8pending = true;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (b->timing) {
        if (b->events.size() < VISO_EVENT_POOL) {
            HIP_TRY(hipEventCreate(&e0));
            HIP_TRY(hipEventCreate(&e1));
            b->events.push_back({e0, e1});
        } else {   // pool full: fold the oldest pair into the running sum (waits for that run) and reuse it
            auto& e = b->events[b->ev_next];
            float ms = 0;
            HIP_TRY(hipEventSynchronize(e.second));
            if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) { b->ev_ms_sum += ms; ++b->ev_n; }
            e0 = e.first; e1 = e.second;
            b->ev_next = (b->ev_next + 1) % VISO_EVENT_POOL;
        }
    }
    VISO_TRY(launch_match(s, b->probs, b->n_probs, b->cap, b->dlen, b->mp, b->bad_any, e0, e1, 1, b->ctx->matcher_variant, b->ovf_q, b->ovf_cnt, r8s, from_images ? 0 : 1));
    VISO_TRY(launch_sort(s, b->probs, b->n_probs, b->cap));
    b->uv_mode = 0;
    if (from_images && b->subpix) {   // the stereo lists are final: refine their right-image points (which = 0 lists come first)
        const SubpixLists lists = {b->kp, 2 * (size_t)b->cap, b->cap, b->sorted, 3 * (size_t)b->cap, b->m_cnt};
        const SubpixLeftRows left = {b->packed, 2 * (size_t)b->cap * VISO_ROW, b->rank, 2 * (size_t)b->cap};
        VISO_TRY(launch_subpixel(s, batch_images(b, 0, b->nf), lists, b->subpix, b->uv, left));
        b->uv_mode = b->subpix;
    }
    if (b->stamps) HIP_TRY(hipEventRecord(b->ev_stamp[2], s));   // re-recorded behind the solver by run_rest
    b->has_run = true;
    return VISO_OK;
}

// Time stamps of a run: which = 0 before the run's uploads, 1 after them (both on the context's stream); the end of
// the run is stamped by viso_batch_run* itself once stamping is on (i.e. after the first viso_batch_stamp call).
extern "C" int viso_batch_stamp(viso_batch* b, int which) {
    if (dead(b) || which < 0 || which > 1) { viso_set_error("viso_batch_stamp: bad argument"); return VISO_ERR_ARG; }
    VISO_TRY(enter(b));
    for (int k = 0; k < 3; ++k)
        if (!b->ev_stamp[k]) HIP_TRY(hipEventCreate(&b->ev_stamp[k]));
    if (!b->stamps) {   // all three recorded once, so that viso_batch_stamp_ms never meets an unrecorded event
        for (int k = 0; k < 3; ++k) HIP_TRY(hipEventRecord(b->ev_stamp[k], b->ctx->stream));
        b->stamps = true;
    }
    HIP_TRY(hipEventRecord(b->ev_stamp[which], b->ctx->stream));
    return VISO_OK;
}

// Waits for the batch; ms[0] = stamp 0 -> stamp 1 (the uploads), ms[1] = stamp 1 -> behind the run's last kernel.
extern "C" int viso_batch_stamp_ms(viso_batch* b, double ms[2]) {
    if (dead(b) || !ms || !b->stamps) { viso_set_error("viso_batch_stamp_ms: no stamps taken"); return VISO_ERR_ARG; }
    VISO_TRY(batch_sync(b));
    float a = 0, c = 0;
    HIP_TRY(hipEventElapsedTime(&a, b->ev_stamp[0], b->ev_stamp[1]));
    HIP_TRY(hipEventElapsedTime(&c, b->ev_stamp[1], b->ev_stamp[2]));
    ms[0] = a; ms[1] = c;
    return VISO_OK;
}

static int run_rest(viso_batch* b) {
    VISO_TRY(enter(b));
    hipStream_t s = b->ctx->stream;
    hipStream_t ss = b->solver_stream ? b->solver_stream : s;
    // the circle join rewrites what the previous run's RANSAC reads (x_c, Xp_c, mc)
    if (ss != s && b->ransac_pending) HIP_TRY(hipStreamWaitEvent(s, b->ev_ransac, 0));
    if (b->nf > 1) {
        VISO_TRY(launch_circle_join(s, b->join, b->nf - 1, b->sp, b->uv_mode != 0));   // :1245-1247 (the rows it joins), :1282, 1292-1305
        if (ss != s) {
            HIP_TRY(hipEventRecord(b->ev_join, s));
            HIP_TRY(hipStreamWaitEvent(ss, b->ev_join, 0));
        }
        // vector<double> tr(6,0), :1312: ransac_refit_kernel writes the zeros itself where no solve succeeds
        VISO_TRY(launch_ransac(ss, b->sitems, b->nf - 1, b->iters, b->seed, b->sp, b->hq, b->ctx->gn_split, b->cap));   // :1313
        // the run's poses, flags and inlier counts into the pinned mirror (the kernel writes over PCIe; viso_batch_get_poses
        // waits for the streams and reads host memory)
        VISO_TRY(plain_blit(ss, b->tr, b->pose_pin, b->pose_bytes / 4));
        VISO_TRY(batch_launch_estimators(b, ss));
    }
    b->est.cov.last = b->est.cov.mode;
    b->est.ref.last = b->est.ref.mode;
    b->est.win.last = b->est.win_K;
    if (ss != s) {
        HIP_TRY(hipEventRecord(b->ev_ransac, ss));
        b->ransac_pending = true;
    }
    if (b->stamps) HIP_TRY(hipEventRecord(b->ev_stamp[2], ss));
    return VISO_OK;
}

extern "C" int viso_batch_run_matcher(viso_batch* b) {
    VISO_TRY(run_matcher_check(b, false));
    return run_matcher_launch(b, false);
}

extern "C" int viso_batch_run(viso_batch* b) {
    VISO_TRY(viso_batch_run_matcher(b));
    return run_rest(b);
}

// Dense disparity (when on) goes on the context's stream behind everything else of the run: the circle join and the RANSAC stream
// are issued first, so the poses do not queue behind it, and it stays outside the run's time stamps.
extern "C" int viso_batch_run_images(viso_batch* b, int matcher_only) {
    const char* where = "viso_batch_run_images";
    VISO_TRY(run_matcher_check(b, true));
    if (b->dense.on()) VISO_TRY(dense_preflight(b, where));
    VISO_TRY(run_matcher_launch(b, true));
    if (!matcher_only) VISO_TRY(run_rest(b));
    return b->dense.on() ? launch_batch_disparity(b, where) : VISO_OK;
}

// HarrisBinnedFeatureDetector on every uploaded image (src/viso.cpp:1226-1227): fills the batch's
// keypoint arrays and counts on the device; viso_batch_run_images then extracts descriptors there too.
extern "C" int viso_batch_detect(viso_batch* b, int n_features, int nbinx, int nbiny, double k) {
    if (dead(b) || !b->images) { viso_set_error("viso_batch_detect: no images uploaded"); return VISO_ERR_ARG; }
    if (n_features < 0 || nbinx <= 0 || nbiny <= 0 || b->img_cols / nbinx <= 0 || b->img_rows / nbiny <= 0 ||
        (long long)nbinx * nbiny > 16384) {
        viso_set_error("viso_batch_detect: bad bin geometry");
        return VISO_ERR_ARG;
    }
    const int nbins = nbinx * nbiny, per = n_features / nbins;
    if ((long long)nbins * per > b->cap) { viso_set_error("viso_batch_detect: %d features exceed the batch capacity %d", nbins * per, b->cap); return VISO_ERR_ARG; }
    const int n_img = b->nf * 2;
    VISO_TRY(enter(b));
    hipStream_t s = b->ctx->stream;
    const bool fused = harris_fused_lds(b->img_rows, b->img_cols, nbinx, nbiny, per) != 0;   // no response image then
    if (!fused && !b->h_resp) VISO_TRY(b->alloc(&b->h_resp, (size_t)n_img * b->img_rows * b->img_cols));
    const size_t slots = (size_t)nbins * (per > 0 ? per : 1);
    if (slots > b->h_slots) {
        HIP_TRY(hipStreamSynchronize(s));
        VISO_TRY(b->release(&b->h_tmp_kp)); VISO_TRY(b->release(&b->h_tmp_resp)); VISO_TRY(b->release(&b->h_cnt));
        VISO_TRY(b->alloc(&b->h_tmp_kp, slots * n_img));
        VISO_TRY(b->alloc(&b->h_tmp_resp, slots * n_img));
        VISO_TRY(b->alloc(&b->h_cnt, (size_t)16384 * n_img));
        b->h_slots = slots;
    }
    if (per == 0) { HIP_TRY(hipMemsetAsync(b->n, 0, sizeof(int) * (size_t)n_img, s)); return VISO_OK; }
    const StereoImages im = batch_images(b, 0, b->nf);
    const HarrisBins bins = {n_features, nbinx, nbiny};
    const HarrisOut out = {b->kp, nullptr, b->n, b->cap, (size_t)b->cap};
    if (fused) {
        const size_t pb = harris_strip_bytes(n_img, b->img_rows, b->img_cols, nbinx, nbiny, per);   // 0: the wave-per-bin kernel
        if (pb) VISO_TRY(b->fit(&b->h_part, &b->h_part_bytes, pb, true));   // grows only
        return launch_harris_detect(s, im, bins, k, HarrisScratch{b->h_tmp_kp, b->h_tmp_resp, b->h_cnt, pb ? b->h_part : nullptr}, out);
    }
    VISO_TRY(launch_harris_response(s, im, k, b->h_resp));
    return launch_harris_bins(s, b->h_resp, im, bins, HarrisScratch{b->h_tmp_kp, b->h_tmp_resp, b->h_cnt, nullptr}, out);
}

// Keypoints of frame t, image side (after viso_batch_detect or an upload).
extern "C" int viso_batch_get_keypoints(viso_batch* b, int t, int side, float* kp, int* n_out) {
    if (dead(b) || t < 0 || t >= b->nf || side < 0 || side > 1 || !n_out) { viso_set_error("viso_batch_get_keypoints: bad argument"); return VISO_ERR_ARG; }
    VISO_TRY(batch_sync(b));
    int n = 0;
    HIP_TRY(hipMemcpy(&n, b->n + (size_t)t * 2 + side, sizeof(int), hipMemcpyDeviceToHost));
    if (n > 0 && kp) HIP_TRY(hipMemcpy(kp, b->kp + ((size_t)t * 2 + side) * b->cap, sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost));
    *n_out = n;
    return VISO_OK;
}

// Opt-in sub-pixel refinement of the stereo observations (not in the reference; subpixel.hip).  The buffer of the refined points
// is allocated on the first request, and the join items are rebuilt to point at it (after the batch's work in flight).
extern "C" int viso_batch_set_subpixel(viso_batch* b, int mode) {
    if (dead(b) || mode < 0 || mode > 2) { viso_set_error("viso_batch_set_subpixel: bad argument (mode 0, 1 or 2)"); return VISO_ERR_ARG; }
    VISO_TRY(enter(b));
    if (mode && !b->uv) {
        VISO_TRY(batch_sync(b));
        VISO_TRY(b->alloc(&b->uv, (size_t)b->nf * b->cap));
        VISO_TRY(build_items(b));
    }
    b->subpix = mode;
    return VISO_OK;
}

// The refined (uR', vR') of frame t's stereo rows, in the order of viso_batch_get_matches(b, 0, t).
extern "C" int viso_batch_get_subpixel(viso_batch* b, int t, float* uv, int* out_n) {
    if (!slot_ok(b, 0, t) || !out_n) { viso_set_error("viso_batch_get_subpixel: bad argument"); return VISO_ERR_ARG; }
    VISO_TRY(batch_sync(b));
    if (!b->uv_mode) { viso_set_error("viso_batch_get_subpixel: the last run refined nothing (mode 0, or not viso_batch_run_images)"); return VISO_ERR_ARG; }
    int m = 0;
    HIP_TRY(hipMemcpy(&m, b->m_cnt + t, sizeof(int), hipMemcpyDeviceToHost));
    if (m > b->cap) m = b->cap;
    if (m > 0 && uv) HIP_TRY(hipMemcpy(uv, b->uv + (size_t)t * b->cap, sizeof(float2) * (size_t)m, hipMemcpyDeviceToHost));
    *out_n = m;
    return VISO_OK;
}

// Frame t's solver inputs (what the circle join wrote for the last run): Xp_c and x_c rows of cap doubles.
extern "C" int viso_batch_get_points(viso_batch* b, int t, double* X3xcap, double* obs4xcap, int* m) {
    if (!slot_ok(b, 0, t) || !m) { viso_set_error("viso_batch_get_points: bad argument"); return VISO_ERR_ARG; }
    VISO_TRY(batch_sync(b));
    int mm = 0;
    HIP_TRY(hipMemcpy(&mm, b->mc + t, sizeof(int), hipMemcpyDeviceToHost));
    mm = mm < 0 ? 0 : mm > b->cap ? b->cap : mm;
    const size_t c = (size_t)b->cap;
    if (X3xcap) HIP_TRY(hipMemcpy(X3xcap, b->Xp_c + (size_t)t * 3 * c, sizeof(double) * 3 * c, hipMemcpyDeviceToHost));
    if (obs4xcap) HIP_TRY(hipMemcpy(obs4xcap, b->x_c + (size_t)t * 4 * c, sizeof(double) * 4 * c, hipMemcpyDeviceToHost));
    *m = mm;
    return VISO_OK;
}

// The geometry of the batch's device images (what viso_batch_get_image copies): 0 x 0 before the first image upload.
extern "C" int viso_batch_get_image_geometry(viso_batch* b, int* rows, int* cols) {
    if (dead(b) || !rows || !cols) { viso_set_error("viso_batch_get_image_geometry: bad argument"); return VISO_ERR_ARG; }
    *rows = b->images ? b->img_rows : 0;
    *cols = b->images ? b->img_cols : 0;
    return VISO_OK;
}

// The device image of frame t, side (what the run reads: rectified when rectification was on at its upload).
extern "C" int viso_batch_get_image(viso_batch* b, int t, int side, uint8_t* out) {
    if (dead(b) || t < 0 || t >= b->nf || side < 0 || side > 1 || !out) { viso_set_error("viso_batch_get_image: bad argument"); return VISO_ERR_ARG; }
    if (!b->images) { viso_set_error("viso_batch_get_image: no images uploaded"); return VISO_ERR_ARG; }
    VISO_TRY(batch_sync(b));
    const size_t per = (size_t)b->img_rows * b->img_cols;
    HIP_TRY(hipMemcpy(out, b->images + ((size_t)t * 2 + side) * per, per, hipMemcpyDeviceToHost));
    return VISO_OK;
}

extern "C" int viso_batch_kernel_ms(viso_batch* b, double* matcher_ms_avg, int* n_launches) {
    if (dead(b)) return VISO_ERR_ARG;
    VISO_TRY(batch_sync(b));
    double tot = b->ev_ms_sum;
    int n = b->ev_n;
    for (auto& e : b->events) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) { tot += ms; ++n; }   // folded pairs were re-recorded since
        hipEventDestroy(e.first); hipEventDestroy(e.second);
    }
    b->events.clear();
    b->ev_next = 0; b->ev_ms_sum = 0; b->ev_n = 0;
    if (matcher_ms_avg) *matcher_ms_avg = n ? tot / n : 0.0;
    if (n_launches) *n_launches = n;
    return VISO_OK;
}

extern "C" int viso_batch_get_matches(viso_batch* b, int which, int t, int32_t* out_match, int* out_n) {
    if (!slot_ok(b, which, t) || !out_n) { viso_set_error("viso_batch_get_matches: bad argument"); return VISO_ERR_ARG; }
    VISO_TRY(batch_sync(b));
    const size_t o = (size_t)which * b->nf + t;
    int m = 0;
    HIP_TRY(hipMemcpy(&m, b->m_cnt + o, sizeof(int), hipMemcpyDeviceToHost));
    if (m > 0 && out_match) HIP_TRY(hipMemcpy(out_match, b->sorted + o * b->cap * 3, sizeof(int) * 3 * (size_t)m, hipMemcpyDeviceToHost));
    *out_n = m;
    return VISO_OK;
}

extern "C" int viso_batch_get_circle(viso_batch* b, int t, int32_t* circ, int32_t* pcl, int* out_n) {
    if (!slot_ok(b, 0, t) || !out_n) { viso_set_error("viso_batch_get_circle: bad argument"); return VISO_ERR_ARG; }
    VISO_TRY(batch_sync(b));
    int m = 0;
    HIP_TRY(hipMemcpy(&m, b->mc + t, sizeof(int), hipMemcpyDeviceToHost));
    if (m > 0 && circ) HIP_TRY(hipMemcpy(circ, b->circ + (size_t)t * b->cap * 4, sizeof(int) * 4 * (size_t)m, hipMemcpyDeviceToHost));
    if (m > 0 && pcl) HIP_TRY(hipMemcpy(pcl, b->pcl + (size_t)t * b->cap * 2, sizeof(int) * 2 * (size_t)m, hipMemcpyDeviceToHost));
    *out_n = m;
    return VISO_OK;
}

extern "C" int viso_batch_get_pose(viso_batch* b, int t, double tr[6], int* ok, int32_t* inliers, int* n_inl) {
    if (!slot_ok(b, 0, t)) { viso_set_error("viso_batch_get_pose: bad argument"); return VISO_ERR_ARG; }
    VISO_TRY(batch_sync(b));
    int o = 0, n = 0;
    const size_t nf = (size_t)b->nf;
    if (tr) memcpy(tr, b->pose_pin + sizeof(double) * 6 * (size_t)t, sizeof(double) * 6);
    memcpy(&o, b->pose_pin + sizeof(double) * 6 * nf + sizeof(int) * (size_t)t, sizeof(int));
    memcpy(&n, b->pose_pin + sizeof(double) * 6 * nf + sizeof(int) * (nf + (size_t)t), sizeof(int));
    if (n > 0 && inliers) HIP_TRY(hipMemcpy(inliers, b->inl + (size_t)t * b->cap, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    if (ok) *ok = o;
    if (n_inl) *n_inl = n;
    return VISO_OK;
}

extern "C" int viso_batch_get_poses(viso_batch* b, double* tr, int32_t* ok, int32_t* n_inl) {
    if (dead(b)) return VISO_ERR_ARG;
    VISO_TRY(batch_sync(b));
    // the pinned mirror of the device block (run_rest's last kernel; zeros before the first run, like the device's)
    const size_t nf = (size_t)b->nf;
    if (tr) memcpy(tr, b->pose_pin, sizeof(double) * 6 * nf);
    if (ok) memcpy(ok, b->pose_pin + sizeof(double) * 6 * nf, sizeof(int) * nf);
    if (n_inl) memcpy(n_inl, b->pose_pin + sizeof(double) * 6 * nf + sizeof(int) * nf, sizeof(int) * nf);
    return VISO_OK;
}

// The per-hypothesis state of the last run's RANSAC stage (test / diagnostics): tr_h [n_frames][iters][6], ok_h and
// cnt_h [n_frames][iters] (frame 0 unused), *n_undecided = hypotheses the lane-per-hypothesis kernel handed on.
extern "C" int viso_batch_get_hypotheses2(viso_batch* b, int capacity, double* tr_h, int32_t* ok_h, int32_t* cnt_h,
                                          int32_t* n_undecided) {
    if (dead(b)) { viso_set_error("viso_batch_get_hypotheses2: bad argument"); return VISO_ERR_ARG; }   // b is not read: it may be freed memory
    const int iters = b->iters > 0 ? b->iters : 1;
    if (capacity < iters) {
        viso_set_error("viso_batch_get_hypotheses2: arrays hold %d hypotheses per frame, the batch has %d", capacity, b->iters);
        return VISO_ERR_ARG;
    }
    if (capacity == iters) return viso_batch_get_hypotheses(b, tr_h, ok_h, cnt_h, n_undecided);
    // the caller's rows are longer than the batch's: frame by frame, at the caller's stride
    if (!b->tr_h) { viso_set_error("viso_batch_get_hypotheses2: no run yet"); return VISO_ERR_ARG; }
    VISO_TRY(batch_sync(b));
    const size_t nf = (size_t)b->nf;
    if (tr_h) HIP_TRY(hipMemcpy2D(tr_h, sizeof(double) * 6 * (size_t)capacity, b->tr_h, sizeof(double) * 6 * (size_t)iters,
                                  sizeof(double) * 6 * (size_t)iters, nf, hipMemcpyDeviceToHost));
    if (ok_h) HIP_TRY(hipMemcpy2D(ok_h, sizeof(int) * (size_t)capacity, b->ok_h, sizeof(int) * (size_t)iters, sizeof(int) * (size_t)iters, nf,
                                  hipMemcpyDeviceToHost));
    if (cnt_h) HIP_TRY(hipMemcpy2D(cnt_h, sizeof(int) * (size_t)capacity, b->cnt_h, sizeof(int) * (size_t)iters, sizeof(int) * (size_t)iters, nf,
                                   hipMemcpyDeviceToHost));
    if (n_undecided) HIP_TRY(hipMemcpy(n_undecided, b->hq + 1, sizeof(int), hipMemcpyDeviceToHost));   // [1]: the last chain's count (solver.hip)
    return VISO_OK;
}

extern "C" int viso_batch_get_hypotheses(viso_batch* b, double* tr_h, int32_t* ok_h, int32_t* cnt_h, int32_t* n_undecided) {
    if (dead(b) || !b->tr_h) { viso_set_error("viso_batch_get_hypotheses: no run yet"); return VISO_ERR_ARG; }
    VISO_TRY(batch_sync(b));
    const size_t k = (size_t)b->nf * (size_t)(b->iters > 0 ? b->iters : 1);
    if (tr_h) HIP_TRY(hipMemcpy(tr_h, b->tr_h, sizeof(double) * 6 * k, hipMemcpyDeviceToHost));
    if (ok_h) HIP_TRY(hipMemcpy(ok_h, b->ok_h, sizeof(int) * k, hipMemcpyDeviceToHost));
    if (cnt_h) HIP_TRY(hipMemcpy(cnt_h, b->cnt_h, sizeof(int) * k, hipMemcpyDeviceToHost));
    if (n_undecided) HIP_TRY(hipMemcpy(n_undecided, b->hq + 1, sizeof(int), hipMemcpyDeviceToHost));   // [1]: the last chain's count (solver.hip)
    return VISO_OK;
}

// Which images the pack kernel flagged in the last run (descriptor values that are not integers in
// [-32768, 32767]): the problems reading them took the general (double) kernel, all others the u16 kernels.
extern "C" int viso_batch_get_general_path_flags(viso_batch* b, int32_t* flags) {
    if (dead(b) || !flags) return VISO_ERR_ARG;
    VISO_TRY(batch_sync(b));
    HIP_TRY(hipMemcpy(flags, b->bad_img, sizeof(int) * 2 * (size_t)b->nf, hipMemcpyDeviceToHost));
    return VISO_OK;
}

// How many queries of the last run the tile kernels handed to match_overflow_kernel (more than K in-radius
// candidates, a candidate list that outgrew its LDS slot, an exact tie of the minimum): the data-dependent slow path.
extern "C" int viso_batch_get_overflow_count(viso_batch* b, int32_t* n) {
    if (dead(b) || !n) return VISO_ERR_ARG;
    VISO_TRY(batch_sync(b));
    HIP_TRY(hipMemcpy(n, b->ovf_cnt, sizeof(int), hipMemcpyDeviceToHost));
    return VISO_OK;
}

extern "C" int viso_batch_get_counters(viso_batch* b, int64_t* scored, int64_t* m_out) {
    if (dead(b)) return VISO_ERR_ARG;
    VISO_TRY(batch_sync(b));
    const size_t k = 3 * (size_t)b->nf;
    if (scored) HIP_TRY(hipMemcpy(scored, b->scored, sizeof(int64_t) * k, hipMemcpyDeviceToHost));
    if (m_out) {
        std::vector<int> m(k);
        HIP_TRY(hipMemcpy(m.data(), b->m_cnt, sizeof(int) * k, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < k; ++i) m_out[i] = m[i];
    }
    return VISO_OK;
}
