// voxel_host.hip — the host side of the shared table layer (voxel_host.h): the registry of live handles, the life of a table, a
// call's scratch block, the staging (the map, the poses and, where a kind fuses one, the image) and the group loop of a fuse
// (as the steps that a retract takes as well),
// the wait behind a call's launches, the pass of an extraction, the staging and the output buffer of a render, the staging and the sums of a linearise, the read-back of the
// statistics, and of an eviction the argument checks, the statistics' round trip and the box around a point.
// No kernel is here: a kind passes in the launches of its own kernels, and the templates of voxel_host.h start the shared ones.
#include "voxel_host.h"

#include <climits>
#include <cmath>
#include <vector>

bool voxel_known(VoxelRegistry& reg, const void* handle) {
    std::lock_guard<std::mutex> lk(reg.mu);
    return handle && reg.live.count(handle) != 0;
}

static bool voxel_ctx_live(const VoxelHost* h) { return viso_ctx_live(h->ctx) && h->ctx->serial == h->ctx_serial; }

static int voxel_not_live(const char* where, const VoxelRegistry& reg) {
    viso_set_error("%s: not a live %s handle", where, reg.kind.handle);
    return VISO_ERR_ARG;
}

int voxel_enter(const char* where, VoxelRegistry& reg, const void* handle, VoxelHost** h) {
    {
        std::lock_guard<std::mutex> lk(reg.mu);
        const auto it = handle ? reg.live.find(handle) : reg.live.end();
        if (it == reg.live.end()) return voxel_not_live(where, reg);
        *h = it->second;
    }
    if (!voxel_ctx_live(*h)) { viso_set_error("%s: the %s's context has been destroyed", where, reg.kind.noun); return VISO_ERR_ARG; }
    HIP_TRY(hipSetDevice((*h)->device));
    return VISO_OK;
}

int voxel_refuse_overflowed(const char* where, const VoxelHost* h) {
    viso_set_error("%s: the %s has overflowed (%s were dropped; which ones depends on scheduling): %s it, or use a larger capacity_log2", where,
                   h->kind->noun, h->kind->unit, h->kind->clear_fn);
    return VISO_ERR_NOMEM;
}

int voxel_create(const char* where, VoxelRegistry& reg, viso_ctx* ctx_or_null, int capacity_log2, int min_disp16, size_t payload_bytes,
                 VoxelHost* h, char** payload) {
    viso_ctx* c;
    VISO_TRY(ctx_resolve(where, ctx_or_null, &c));
    HIP_TRY(hipSetDevice(c->device));
    const size_t slots = (size_t)1 << capacity_log2;
    const size_t b_keys = 8 * slots, b_payload = payload_bytes * slots, b_stats = 8 * VOXEL_STAT_SETS * VOXEL_STAT_WORDS;
    const size_t b_words = 256;
    static_assert(VOXEL_WORDS * sizeof(unsigned long long) <= b_words, "the clear kernel zeroes VOXEL_WORDS words behind the stats");
    const size_t bytes = b_keys + b_payload + b_stats + b_words;
    void* block = nullptr;
    if (hipMalloc(&block, bytes) != hipSuccess) {
        (void)hipGetLastError();
        viso_set_error("%s: cannot allocate the %zu-byte table of 2^%d slots", where, bytes, capacity_log2);
        return VISO_ERR_NOMEM;
    }
    h->kind = &reg.kind;
    h->ctx = c; h->ctx_serial = c->serial; h->device = c->device;
    h->capacity_log2 = capacity_log2; h->min_disp16 = min_disp16;
    h->block = block;
    char* at = static_cast<char*>(block);
    h->head.keys = reinterpret_cast<unsigned long long*>(at); at += b_keys;
    *payload = at; at += b_payload;
    h->head.stats = reinterpret_cast<unsigned long long*>(at); at += b_stats;
    h->head.words = reinterpret_cast<unsigned long long*>(at);
    h->head.mask = (uint32_t)(slots - 1);
    h->overflowed = false;
    h->d_disp = nullptr; h->d_disp_bytes = 0; h->d_image = nullptr; h->d_image_bytes = 0; h->d_pose = nullptr; h->d_pose_bytes = 0;
    return VISO_OK;
}

static int voxel_launch_clear(VoxelHost* h, const VoxelLaunch& clear) {
    clear(h->ctx->stream);
    HIP_TRY(hipGetLastError());
    h->overflowed = false;
    return VISO_OK;
}

int voxel_open(VoxelRegistry& reg, const void* handle, VoxelHost* h, const VoxelLaunch& clear) {
    const int r = voxel_launch_clear(h, clear);
    if (r < 0) { (void)hipFree(h->block); return r; }
    std::lock_guard<std::mutex> lk(reg.mu);
    reg.live[handle] = h;
    return VISO_OK;
}

bool voxel_unregister(const char* where, VoxelRegistry& reg, const void* handle) {
    std::lock_guard<std::mutex> lk(reg.mu);
    if (reg.live.erase(handle)) return true;
    voxel_not_live(where, reg);
    return false;
}

int voxel_free(const char* where, VoxelHost* h) {
    hipError_t first = hipSetDevice(h->device);
    auto note = [&](hipError_t e) { if (e != hipSuccess && first == hipSuccess) first = e; };
    if (voxel_ctx_live(h)) note(hipStreamSynchronize(h->ctx->stream));   // a destroyed context has waited for its streams itself
    note(hipFree(h->block));
    if (h->d_disp) note(hipFree(h->d_disp));
    if (h->d_image) note(hipFree(h->d_image));
    if (h->d_pose) note(hipFree(h->d_pose));
    if (first != hipSuccess) { viso_set_error("%s: %s", where, hipGetErrorString(first)); return VISO_ERR_HIP; }
    return VISO_OK;
}

int voxel_clear(const char* where, VoxelRegistry& reg, const void* handle, const VoxelLaunch& clear) {
    VoxelSession ses(where, reg, handle, VoxelSession::ANY_STATE);
    VISO_TRY(ses.status());
    return voxel_launch_clear(ses.host(), clear);
}

VoxelScratch::VoxelScratch(const VoxelSession& ses, size_t bytes, const char* what) : stream_(ses.stream()) {
    if (!bytes || hipMalloc((void**)&d_, bytes) == hipSuccess) return;
    (void)hipGetLastError();
    d_ = nullptr;
    viso_set_error("%s: cannot allocate %zu bytes for %s", ses.where(), bytes, what);
    status_ = VISO_ERR_NOMEM;
}

int VoxelScratch::release() {
    if (released_) return VISO_OK;
    released_ = true;
    const hipError_t e_wait = hipStreamSynchronize(stream_);   // nothing in flight touches the block that is freed next
    if (d_) (void)hipFree(d_);
    d_ = nullptr;
    HIP_TRY(e_wait);
    return VISO_OK;
}

// grow-only staging of `bytes` at *p
template <class T>
static int voxel_grow(const char* where, T** p, size_t* have, size_t bytes, hipStream_t s) {
    if (*have >= bytes) return VISO_OK;
    HIP_TRY(hipStreamSynchronize(s));   // nothing in flight reads the old block
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr; *have = 0;
    if (hipMalloc((void**)p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        viso_set_error("%s: cannot allocate %zu bytes of staging", where, bytes);
        return VISO_ERR_NOMEM;
    }
    *have = bytes;
    return VISO_OK;
}

int voxel_finish(const char* where, VoxelHost* h) {
    unsigned long long dropped = 0;
    hipStream_t s = h->ctx->stream;
    HIP_TRY(hipMemcpyAsync(&dropped, h->head.words + VOXEL_W_DROPPED, sizeof(dropped), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (dropped) {
        h->overflowed = true;
        viso_set_error("%s: the table of 2^%d slots is full: %llu %s found no slot (%s, or a larger capacity_log2)", where, h->capacity_log2,
                       dropped, h->kind->unit, h->kind->clear_fn);
        return VISO_ERR_NOMEM;
    }
    return VISO_OK;
}

static bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

// Not the alignment's check (tsdf_align.hip, align_check): a fuse only scales and offsets by the calibration, so any finite one
// will do, and the limit on the pixels is this build's 32-bit pixel index, not the definition's: VISO_ERR_UNSUPPORTED.
static int voxel_fuse_check(const char* where, const DispView& v) {
    if (v.poses && !all_finite(v.poses, (size_t)v.n * 16)) { viso_set_error("%s: a pose has an entry that is not finite", where); return VISO_ERR_ARG; }
    if (!std::isfinite(v.cal.f) || !std::isfinite(v.cal.cu) || !std::isfinite(v.cal.cv) || !std::isfinite(v.cal.base)) {
        viso_set_error("%s: the calibration (f, cu, cv, base) must be finite", where);
        return VISO_ERR_ARG;
    }
    if ((long long)v.rows * v.cols > VOXEL_MAX_PIXELS) { viso_set_error("%s: a %d x %d map is beyond this build (2^31 - 1 pixels)", where, v.rows, v.cols); return VISO_ERR_UNSUPPORTED; }
    return VISO_OK;
}

// The first three rows of n poses [n][16] into h->d_pose (grow-only) as [n][12]; rows12 is the copy's source and must live until
// the stream has been waited for.  h is entered and locked.
static int voxel_stage_poses(const char* where, VoxelHost* h, const double* poses, int n, std::vector<double>& rows12) {
    hipStream_t s = h->ctx->stream;
    int r;
    rows12.resize((size_t)n * 12);
    for (int k = 0; k < n; ++k) std::copy(poses + (size_t)k * 16, poses + (size_t)k * 16 + 12, rows12.begin() + (size_t)k * 12);
    if ((r = voxel_grow(where, &h->d_pose, &h->d_pose_bytes, rows12.size() * sizeof(double), s)) < 0) return r;
    HIP_TRY(hipMemcpyAsync(h->d_pose, rows12.data(), rows12.size() * sizeof(double), hipMemcpyHostToDevice, s));
    return VISO_OK;
}

int voxel_fuse_args(const char* where, VoxelRegistry& reg, const void* handle, const DispView& v) {
    if (!voxel_known(reg, handle)) return voxel_not_live(where, reg);
    if (!v.ctx && (!v.disp || v.rows <= 0 || v.cols <= 0)) { viso_set_error("%s: bad argument (non-null map and calibration, sizes > 0)", where); return VISO_ERR_ARG; }
    return voxel_fuse_check(where, v);
}

int voxel_fuse_stage(const VoxelSession& ses, VoxelRegistry& reg, const DispView& v, VoxelFrames* f) {
    const char* where = ses.where();
    VoxelHost* h = ses.host();
    if (v.ctx && h->ctx != v.ctx) { viso_set_error("%s: the %s and the batch must share a context", where, reg.kind.noun); return VISO_ERR_ARG; }
    VISO_TRY(ses.refuse_overflowed());
    int r;
    const size_t px = v.px();
    f->disp = v.disp;
    f->image = v.image;
    if (!v.ctx) {   // one host map, and one host image if there is one, through the staging
        if ((r = voxel_stage_map(where, h, v.disp, px, &f->disp)) < 0) return r;
        if (v.image && (r = voxel_stage_image(where, h, v.image, px, &f->image)) < 0) return r;
    }
    if (v.poses && (r = voxel_stage_poses(where, h, v.poses, v.n, f->rows12)) < 0) return r;
    VoxelFuseArgs& a = f->a;
    a.disp = nullptr; a.poses = nullptr;
    a.mfs = v.mfs; a.rows = v.rows; a.cols = v.cols; a.min_disp16 = h->min_disp16; a._pad = 0;
    a.f = v.cal.f; a.cu = v.cal.cu; a.cv = v.cal.cv; a.base = v.cal.base;
    return VISO_OK;
}

int voxel_fuse_restage(const VoxelSession& ses, const double* poses, int n, VoxelFrames* f) {
    return poses ? voxel_stage_poses(ses.where(), ses.host(), poses, n, f->rows12) : VISO_OK;
}

int voxel_fuse_groups(VoxelHost* h, const DispView& v, const VoxelFrames& f, const VoxelFuseLaunch& launch) {
    hipStream_t s = h->ctx->stream;
    const size_t px = v.px();
    VoxelFuseArgs a = f.a;
    for (int f0 = 0; f0 < v.n; f0 += VOXEL_GROUP) {
        const int nf = v.n - f0 < VOXEL_GROUP ? v.n - f0 : VOXEL_GROUP;
        a.disp = f.disp + (size_t)f0 * v.mfs;
        a.poses = v.poses ? h->d_pose + (size_t)f0 * 12 : nullptr;
        launch(a, f.image ? f.image + (size_t)f0 * v.ifs : nullptr, dim3((unsigned)((px + 255) / 256), (unsigned)nf), s);
        HIP_TRY(hipGetLastError());
    }
    return VISO_OK;
}

int voxel_fuse(const char* where, VoxelRegistry& reg, const void* handle, const DispView& v, const VoxelFuseLaunch& launch) {
    int r;
    if ((r = voxel_fuse_args(where, reg, handle, v)) < 0) return r;
    VoxelSession ses(where, reg, handle, VoxelSession::ANY_STATE);   // the overflow refusal comes behind the context's
    VISO_TRY(ses.status());
    VoxelFrames f;   // its poses are alive until voxel_finish has waited for the copy that reads them
    if ((r = voxel_fuse_stage(ses, reg, v, &f)) < 0) return r;
    if ((r = voxel_fuse_groups(ses.host(), v, f, launch)) < 0) return r;
    return voxel_finish(where, ses.host());
}

int voxel_read_words(VoxelHost* h, int first, int n, unsigned long long* out) {
    hipStream_t s = h->ctx->stream;
    HIP_TRY(hipMemcpyAsync(out, h->head.words + first, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VISO_OK;
}

int voxel_pass(VoxelHost* h, const VoxelLaunch& launch, unsigned long long* n, unsigned long long* n_tris) {
    hipStream_t s = h->ctx->stream;
    HIP_TRY(hipMemsetAsync(h->head.words + VOXEL_W_OUT, 0, sizeof(unsigned long long), s));
    if (n_tris) HIP_TRY(hipMemsetAsync(h->head.words + VOXEL_W_TRIS, 0, sizeof(unsigned long long), s));
    launch(s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(n, h->head.words + VOXEL_W_OUT, sizeof(*n), hipMemcpyDeviceToHost, s));
    if (n_tris) HIP_TRY(hipMemcpyAsync(n_tris, h->head.words + VOXEL_W_TRIS, sizeof(*n_tris), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VISO_OK;
}

bool voxel_evict_args(const char* where, VoxelRegistry& reg, const void* handle, const viso_voxel_box* keep, const size_t* n) {
    if (!voxel_known(reg, handle)) { voxel_not_live(where, reg); return false; }
    bool ok = keep && n;
    for (int i = 0; ok && i < 3; ++i) ok = keep->lo[i] <= keep->hi[i];
    if (!ok) viso_set_error("%s: bad argument (a non-null box with lo <= hi on every axis, a non-null n)", where);
    return ok;
}

unsigned long long voxel_stat_sum(const std::vector<unsigned long long>& stats, int which) {
    unsigned long long sum = 0;
    for (int k = 0; k < VOXEL_STAT_SETS; ++k) sum += stats[(size_t)k * VOXEL_STAT_WORDS + which];
    return sum;
}

int voxel_evict_get_stats(VoxelHost* h, std::vector<unsigned long long>& stats, unsigned long long* occupied) {
    hipStream_t s = h->ctx->stream;
    stats.resize((size_t)VOXEL_STAT_SETS * VOXEL_STAT_WORDS);
    HIP_TRY(hipMemcpyAsync(stats.data(), h->head.stats, stats.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *occupied = voxel_stat_sum(stats, VOXEL_ST_OCC);
    return VISO_OK;
}

// (the caller waits for the stream before `stats` goes)
int voxel_evict_put_stats(VoxelHost* h, std::vector<unsigned long long>& stats, unsigned long long less) {
    for (int k = 0; k < VOXEL_STAT_SETS && less; ++k) {   // a set gives what it has: no counter wraps
        unsigned long long& occ = stats[(size_t)k * VOXEL_STAT_WORDS + VOXEL_ST_OCC];
        const unsigned long long take = occ < less ? occ : less;
        occ -= take; less -= take;
    }
    HIP_TRY(hipMemcpyAsync(h->head.stats, stats.data(), stats.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, h->ctx->stream));
    return VISO_OK;
}

extern "C" int viso_voxel_box_around(const double centre[3], double half_side, double voxel, viso_voxel_box* out) {
    bool ok = centre && out && std::isfinite(half_side) && half_side >= 0.0 && std::isfinite(voxel) && voxel > 0.0;
    for (int i = 0; ok && i < 3; ++i) ok = std::isfinite(centre[i]);
    if (!ok) {
        viso_set_error("viso_voxel_box_around: bad argument (a finite centre, a finite half_side >= 0, a finite voxel > 0, a non-null output)");
        return VISO_ERR_ARG;
    }
    auto clamp32 = [](double g, long long add) {   // (int64) g + add clamped to int32; g is a floor, or an infinity
        if (!(g > -4294967296.0)) return (int32_t)INT32_MIN;
        if (!(g < 4294967296.0)) return (int32_t)INT32_MAX;
        const long long v = (long long)g + add;
        return (int32_t)(v < INT32_MIN ? INT32_MIN : v > INT32_MAX ? INT32_MAX : v);
    };
    for (int i = 0; i < 3; ++i) {
        out->lo[i] = clamp32(std::floor((centre[i] - half_side) / voxel), 0);
        out->hi[i] = clamp32(std::floor((centre[i] + half_side) / voxel), 1);
    }
    return VISO_OK;
}

int voxel_render(const char* where, VoxelRegistry& reg, const void* handle, size_t px, const double* poses, int n_views, const VoxelRenderOut& out,
                 const VoxelRenderLaunch& launch) {
    VoxelSession ses(where, reg, handle);
    VISO_TRY(ses.status());
    VoxelHost* h = ses.host();
    hipStream_t s = ses.stream();
    // bytes a pixel: the normals, then the weights, then the maps, then the intensities
    const size_t per = (out.normals ? 12 : 0) + (out.weight ? 6 : 2) + (out.gray ? 1 : 0);
    if (px > (size_t)-1 / per / (size_t)n_views) { viso_set_error("%s: %d views of %zu pixels are beyond the address space", where, n_views, px); return VISO_ERR_NOMEM; }
    const size_t n = (size_t)n_views * px, b_normals = out.normals ? n * 3 * sizeof(float) : 0, b_weight = out.weight ? n * sizeof(uint32_t) : 0,
                 b_disp = n * sizeof(int16_t), bytes = b_normals + b_weight + b_disp + (out.gray ? n : 0);
    std::vector<double> rows12;   // (before the block: the copy of the poses reads it until the block's wait, a failed allocation's too)
    if (poses) VISO_TRY(voxel_stage_poses(where, h, poses, n_views, rows12));
    VoxelScratch d(ses, bytes, "the views");
    VISO_TRY(d.status());
    float* d_normals = out.normals ? d.as<float>() : nullptr;
    uint32_t* d_weight = out.weight ? d.as<uint32_t>(b_normals) : nullptr;
    int16_t* d_disp = d.as<int16_t>(b_normals + b_weight);
    uint8_t* d_gray = out.gray ? d.as<uint8_t>(b_normals + b_weight + b_disp) : nullptr;
    for (int v0 = 0; v0 < n_views; v0 += VOXEL_GROUP) {
        const int nv = n_views - v0 < VOXEL_GROUP ? n_views - v0 : VOXEL_GROUP;
        launch(poses ? h->d_pose + (size_t)v0 * 12 : nullptr, d_disp + (size_t)v0 * px, d_weight ? d_weight + (size_t)v0 * px : nullptr,
               d_gray ? d_gray + (size_t)v0 * px : nullptr, d_normals ? d_normals + (size_t)v0 * px * 3 : nullptr, dim3((unsigned)((px + 255) / 256), (unsigned)nv), s);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(out.disp, d_disp, n * sizeof(int16_t), hipMemcpyDeviceToHost, s));
    if (d_weight) HIP_TRY(hipMemcpyAsync(out.weight, d_weight, b_weight, hipMemcpyDeviceToHost, s));
    if (d_gray) HIP_TRY(hipMemcpyAsync(out.gray, d_gray, n, hipMemcpyDeviceToHost, s));
    if (d_normals) HIP_TRY(hipMemcpyAsync(out.normals, d_normals, b_normals, hipMemcpyDeviceToHost, s));
    return d.release();
}

int voxel_stage_map(const char* where, VoxelHost* h, const int16_t* disp, size_t px, const int16_t** d_disp) {
    hipStream_t s = h->ctx->stream;
    int r;
    if ((r = voxel_grow(where, &h->d_disp, &h->d_disp_bytes, px * sizeof(int16_t), s)) < 0) return r;
    HIP_TRY(hipMemcpyAsync(h->d_disp, disp, px * sizeof(int16_t), hipMemcpyHostToDevice, s));
    *d_disp = h->d_disp;
    return VISO_OK;
}

int voxel_stage_image(const char* where, VoxelHost* h, const uint8_t* image, size_t px, const uint8_t** d_image) {
    hipStream_t s = h->ctx->stream;
    int r;
    if ((r = voxel_grow(where, &h->d_image, &h->d_image_bytes, px, s)) < 0) return r;
    HIP_TRY(hipMemcpyAsync(h->d_image, image, px, hipMemcpyHostToDevice, s));
    *d_image = h->d_image;
    return VISO_OK;
}

int voxel_linearize(const char* where, VoxelHost* h, const double* poses, const unsigned long long* active, int n, size_t words,
                    unsigned long long* out, const VoxelLinearizeLaunch& launch) {
    hipStream_t s = h->ctx->stream;
    int r;
    // one block: poses [n][12] | active [n] | sums [n][words], all 8-byte words; the first two staged with one copy
    std::vector<double> stage((size_t)n * 13);
    for (int k = 0; k < n; ++k) std::copy(poses + (size_t)k * 16, poses + (size_t)k * 16 + 12, stage.begin() + (size_t)k * 12);
    std::copy(active, active + n, reinterpret_cast<unsigned long long*>(stage.data() + (size_t)n * 12));
    const size_t b_stage = stage.size() * sizeof(double), b_out = (size_t)n * words * sizeof(unsigned long long);
    if ((r = voxel_grow(where, &h->d_pose, &h->d_pose_bytes, b_stage + b_out, s)) < 0) return r;
    const double* d_poses = h->d_pose;
    const unsigned long long* d_active = reinterpret_cast<const unsigned long long*>(h->d_pose + (size_t)n * 12);
    unsigned long long* d_out = reinterpret_cast<unsigned long long*>(h->d_pose + (size_t)n * 13);
    hipError_t e = hipMemcpyAsync(h->d_pose, stage.data(), b_stage, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_out, 0, b_out, s);
    for (int f0 = 0; f0 < n && e == hipSuccess; f0 += VOXEL_GROUP) {
        const int nf = n - f0 < VOXEL_GROUP ? n - f0 : VOXEL_GROUP;
        launch(d_poses + (size_t)f0 * 12, d_active + f0, d_out + (size_t)f0 * words, f0, (unsigned)nf, s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, b_out, hipMemcpyDeviceToHost, s);
    const hipError_t e_wait = hipStreamSynchronize(s);   // the copies read `stage` and write `out`
    HIP_TRY(e);
    HIP_TRY(e_wait);
    return VISO_OK;
}

int voxel_stats(const char* where, VoxelRegistry& reg, const void* handle, const void* out, unsigned long long sums[4], unsigned long long* dropped) {
    if (!voxel_known(reg, handle)) return voxel_not_live(where, reg);
    if (!out) { viso_set_error("%s: bad argument (a non-null output)", where); return VISO_ERR_ARG; }
    VoxelSession ses(where, reg, handle, VoxelSession::ANY_STATE);
    VISO_TRY(ses.status());
    VoxelHost* h = ses.host();
    std::vector<unsigned long long> w((size_t)VOXEL_STAT_SETS * VOXEL_STAT_WORDS + 2);
    hipStream_t s = h->ctx->stream;
    HIP_TRY(hipMemcpyAsync(w.data(), h->head.stats, w.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));   // stats | words: adjacent
    HIP_TRY(hipStreamSynchronize(s));
    for (int c = 0; c < 4; ++c) {
        sums[c] = 0;
        for (int k = 0; k < VOXEL_STAT_SETS; ++k) sums[c] += w[(size_t)k * VOXEL_STAT_WORDS + c];
    }
    *dropped = w[(size_t)VOXEL_STAT_SETS * VOXEL_STAT_WORDS + VOXEL_W_DROPPED];
    return VISO_OK;
}
