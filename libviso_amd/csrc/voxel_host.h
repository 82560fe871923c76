// voxel_host.h — the host side of the shared table layer of the hash tables of voxels (voxelmap.hip, tsdf.hip; the device side is
// voxel_hash.h; DESIGN.md 5.14, "Shared table layer").  A kind of map (viso_map, viso_tsdf) holds a VoxelHost, has a VoxelRegistry
// of its live handles, and passes in its payload (voxel_hash.h) for the shared kernels and the launches of its own kernels as
// callables.  The rules that every kind must keep are here and in voxel_host.hip, once: no handle is dereferenced before its
// registry has answered for it; staging is freed only behind a synchronise; dropped updates become the sticky overflow mark; an
// eviction and a retract leave no tombstone behind (voxel_finish_removal), and a refused retract leaves every word as it was.  Two of them are types, and every call on a map goes through them:
//   VoxelSession  how a call gets at a map: the registry's answer, the live context, the map's device current (voxel_enter, which
//                 nothing else calls), then the map's mutex for as long as the session lives, then, unless the call asks for a map in
//                 any state (clear, stats, the option calls), the refusal of an overflowed map.  Nothing else locks VoxelHost::mu.
//   VoxelScratch  a call's temporary device block, the only hipMalloc / hipFree outside the life of a table and its staging: the
//                 "cannot allocate" text, and a release (or the destructor, on any return) that waits for the map's stream before
//                 it frees, so nothing in flight touches the block or the host memory a call's copies read and write.
#ifndef VISO_VOXEL_HOST_H_
#define VISO_VOXEL_HOST_H_
#include "voxel_hash.h"

#include <algorithm>
#include <functional>
#include <mutex>
#include <unordered_map>
#include <vector>

// the words of a kind in the error texts
struct VoxelKind {
    const char* handle;      // "map" / "TSDF": "not a live %s handle"
    const char* noun;        // "map" / "TSDF map"
    const char* unit;        // what a full table drops: "points" / "updates"
    const char* threshold;   // the getters' "min_count" / "min_weight"
    const char* clear_fn;    // the function an overflowed map is sent to
};

struct VoxelHost {
    const VoxelKind* kind;
    viso_ctx* ctx; unsigned long long ctx_serial; int device;
    int capacity_log2, min_disp16;
    VoxelTable head; void* block;            // one allocation: keys | payload | stats | words
    bool overflowed;
    int16_t* d_disp; size_t d_disp_bytes;    // staging of a fuse's host map (grow-only)
    uint8_t* d_image; size_t d_image_bytes;  // staging of a fuse's host image (grow-only; a kind that fuses none never has one)
    double* d_pose; size_t d_pose_bytes;     // the poses of a call (grow-only)
    std::mutex mu;
};

// the live handles of one kind, each with the shared state inside it
struct VoxelRegistry {
    const VoxelKind kind;
    std::mutex mu;
    std::unordered_map<const void*, VoxelHost*> live;
};

using VoxelLaunch = std::function<void(hipStream_t)>;                                             // the clear
// one group of frames; d_image: the group's first image on the device, or null when the call has none
using VoxelFuseLaunch = std::function<void(const VoxelFuseArgs&, const uint8_t* d_image, dim3 grid, hipStream_t)>;
// one group of views; d_gray, d_normals: the group's part of the third output, or null when the call has none of that kind
using VoxelRenderLaunch = std::function<void(const double* d_poses, int16_t* d_disp, uint32_t* d_weight, uint8_t* d_gray, float* d_normals, dim3 grid,
                                             hipStream_t)>;
// one group of `frames` frames of a linearise: the group's poses [.][12], its flags and its part of the sums, the group's first
// frame; the grid is the caller's, with the group's frames along y
using VoxelLinearizeLaunch = std::function<void(const double* d_poses, const unsigned long long* d_active, unsigned long long* d_out, int frame0,
                                                unsigned frames, hipStream_t)>;
// what a render writes on the host: n_views maps, with `weight` set as many weights, with `gray` set as many intensities, with
// `normals` set as many times three floats
struct VoxelRenderOut { int16_t* disp; uint32_t* weight; uint8_t* gray; float* normals; };
// where a count or a list goes: *n the number of items; count_only: nothing else, otherwise the items to out[0 .. cap)
template <class Item>
struct VoxelList { bool count_only; Item* out; size_t cap; size_t* n; };

// the launches of voxel_hash.h's kernels over the payload p of a kind: one thread per slot / per entry
template <class P>
void voxel_start_clear(const P& p, hipStream_t s) {
    hipLaunchKernelGGL(voxel_clear_kernel<P>, dim3((p.head().mask + 1u) / 256u), dim3(256), 0, s, p);
}
template <class P>
void voxel_start_add_entries(const P& p, const typename P::Entry* d_entries, unsigned long long n, hipStream_t s) {
    hipLaunchKernelGGL(voxel_add_entries_kernel<P>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, d_entries, n);
}

bool voxel_known(VoxelRegistry& reg, const void* handle);
// a live handle whose context is alive, its device current: *h set; else the error text and code.  Only a VoxelSession calls it.
int voxel_enter(const char* where, VoxelRegistry& reg, const void* handle, VoxelHost** h);
int voxel_refuse_overflowed(const char* where, const VoxelHost* h);

// A call's hold on a map, from voxel_enter to the call's return; the map's mutex is held while the session lives.  status() < 0: the
// call's return value (the error text is set), and nothing else of the session may be used.
class VoxelSession {
public:
    enum State { NOT_OVERFLOWED, ANY_STATE };
    // ANY_STATE: an overflowed map is not refused (a call with checks of its own before that refusal makes it with refuse_overflowed)
    VoxelSession(const char* where, VoxelRegistry& reg, const void* handle, State state = NOT_OVERFLOWED) : where_(where) {
        if ((status_ = voxel_enter(where, reg, handle, &h_)) < 0) return;
        lock_ = std::unique_lock<std::mutex>(h_->mu);
        if (state == NOT_OVERFLOWED) status_ = refuse_overflowed();
    }
    int status() const { return status_; }
    int refuse_overflowed() const { return h_->overflowed ? voxel_refuse_overflowed(where_, h_) : VISO_OK; }
    const char* where() const { return where_; }
    VoxelHost* host() const { return h_; }
    hipStream_t stream() const { return h_->ctx->stream; }

private:
    const char* where_;
    VoxelHost* h_ = nullptr;
    int status_;
    std::unique_lock<std::mutex> lock_;
};

// At most one temporary device block of a session, on its device: `bytes` for `what` ("the list", "the views": the noun of the
// error text); 0 bytes allocate nothing.  release() waits for the map's stream (with a block or without one: an eviction that
// lists nothing still has the copy of its statistics in flight), frees the block and reports a failed wait; the destructor does
// the same where release() was not called, so a call may return wherever it likes.  Host memory that the call's copies read or
// write on the stream is declared before the block: it then outlives the wait.
class VoxelScratch {
public:
    VoxelScratch(const VoxelSession& ses, size_t bytes, const char* what);
    ~VoxelScratch() { (void)release(); }
    VoxelScratch(const VoxelScratch&) = delete;
    VoxelScratch& operator=(const VoxelScratch&) = delete;
    int status() const { return status_; }   // < 0: the call's return value, the error text is set
    template <class T>
    T* as(size_t byte_offset = 0) const { return reinterpret_cast<T*>(d_ + byte_offset); }
    int release();

private:
    hipStream_t stream_;
    char* d_ = nullptr;
    int status_ = VISO_OK;
    bool released_ = false;
};

// viso_*_create behind the check of the parameters.  voxel_create: the context's choice and the table's one allocation of
// 2^capacity_log2 slots with payload_bytes a slot (a multiple of 4, its 8-byte arrays first); h filled, *payload the payload's
// start.  voxel_open, once the caller has set its table up: the first clear, then the handle is live (on failure the table is freed).
int voxel_create(const char* where, VoxelRegistry& reg, viso_ctx* ctx_or_null, int capacity_log2, int min_disp16, size_t payload_bytes,
                 VoxelHost* h, char** payload);
int voxel_open(VoxelRegistry& reg, const void* handle, VoxelHost* h, const VoxelLaunch& clear);
// viso_*_destroy for a non-null handle: voxel_unregister (false: not a live handle, the error text set, nothing touched), then
// voxel_free of everything on the device, then the caller's delete
bool voxel_unregister(const char* where, VoxelRegistry& reg, const void* handle);
int voxel_free(const char* where, VoxelHost* h);
int voxel_clear(const char* where, VoxelRegistry& reg, const void* handle, const VoxelLaunch& clear);

// map_fuse_resident / tsdf_fuse_resident (common.h) and viso_*_fuse, whole, over the view v (common.h) of either kind: the handle
// and argument checks, the staging of the poses and of a host view's map and image, the groups of frames, each started by `launch`
// with its first image (or null), and the wait that finds a full table.
int voxel_fuse(const char* where, VoxelRegistry& reg, const void* handle, const DispView& v, const VoxelFuseLaunch& launch);
// The steps voxel_fuse is made of, for the calls that march the same frames with other launches (voxel_retract):
//   voxel_fuse_args     what is checked before a device is touched: the handle, the view's map and sizes, finite poses and calibration
//   voxel_fuse_stage    under the call's session (opened in ANY_STATE): the batch's context, the overflow refusal, then the staging of
//                       the poses and of a host view's map and image; *f: where the frames lie on the device
//   voxel_fuse_restage  other poses [n][16] (null: none) for the same frames, behind the launches that read the first ones
//   voxel_fuse_groups   the groups of VOXEL_GROUP frames, each started by `launch`; v.poses says whether the groups have poses
struct VoxelFrames {
    VoxelFuseArgs a;                               // all but disp and poses, which a group sets
    const int16_t* disp; const uint8_t* image;     // the first frame's map and image (or null) on the device
    std::vector<double> rows12;                    // what the copy of the poses reads: alive until the stream has been waited for
};
int voxel_fuse_args(const char* where, VoxelRegistry& reg, const void* handle, const DispView& v);
int voxel_fuse_stage(const VoxelSession& ses, VoxelRegistry& reg, const DispView& v, VoxelFrames* f);
int voxel_fuse_restage(const VoxelSession& ses, const double* poses, int n, VoxelFrames* f);
int voxel_fuse_groups(VoxelHost* h, const DispView& v, const VoxelFrames& f, const VoxelFuseLaunch& launch);
// n of the table's words from VOXEL_W_`first` on, behind everything on the map's stream.  h is entered and locked.
int voxel_read_words(VoxelHost* h, int first, int n, unsigned long long* out);
// behind a call's launches: waits for them and turns dropped points / updates into the overflow mark.  h is entered and locked.
int voxel_finish(const char* where, VoxelHost* h);
// viso_*_add_entries behind the handle check and the validation of the n entries
template <class P>
int voxel_add_entries(const char* where, VoxelRegistry& reg, const void* handle, const typename P::Entry* entries, size_t n, const P& p) {
    VoxelSession ses(where, reg, handle);
    VISO_TRY(ses.status());
    if (!n) return VISO_OK;
    hipStream_t s = ses.stream();
    const size_t bytes = n * sizeof(typename P::Entry);
    VoxelScratch d(ses, bytes, "the entries");   // (its wait is also the one behind which the caller's entries are read no more)
    VISO_TRY(d.status());
    HIP_TRY(hipMemcpyAsync(d.as<typename P::Entry>(), entries, bytes, hipMemcpyHostToDevice, s));
    voxel_start_add_entries(p, d.as<typename P::Entry>(), (unsigned long long)n, s);
    HIP_TRY(hipGetLastError());
    return voxel_finish(where, ses.host());
}
// viso_*_render behind the handle and argument checks: a session on the map; the poses [n_views][16] (or null) through d_pose; a
// scratch block for n_views maps of px int16 and, with out.weight, as many uint32, with out.gray, as many uint8, and with
// out.normals, three floats a pixel; the groups of views, each started by `launch` with its poses ([.][12] or null) and its part
// of the block; the copies to the host.
int voxel_render(const char* where, VoxelRegistry& reg, const void* handle, size_t px, const double* poses, int n_views, const VoxelRenderOut& out,
                 const VoxelRenderLaunch& launch);
// A host map of px pixels into the fuse's staging d_disp (grow-only), on the stream; *d_disp: where it is.  h is entered and locked.
int voxel_stage_map(const char* where, VoxelHost* h, const int16_t* disp, size_t px, const int16_t** d_disp);
// The same for a host image of px bytes into d_image (grow-only): the image of a photometric linearise.
int voxel_stage_image(const char* where, VoxelHost* h, const uint8_t* image, size_t px, const uint8_t** d_image);
// One linearise of an alignment (include/viso_hip.h, "TSDF align") for n frames: h is entered, locked and not overflowed (the
// caller holds the lock over the whole alignment).  The poses [n][16] as [n][12], the flags active [n] (0: the frame's lanes
// leave at once) and `words` zeroed 64-bit sums a frame go through d_pose (grow-only), the groups of frames are started by `launch`
// and the sums come back to out [n][words].
int voxel_linearize(const char* where, VoxelHost* h, const double* poses, const unsigned long long* active, int n, size_t words,
                    unsigned long long* out, const VoxelLinearizeLaunch& launch);
// viso_*_stats: the four counters summed over the sets (VOXEL_ST_*) and the dropped word
int voxel_stats(const char* where, VoxelRegistry& reg, const void* handle, const void* out, unsigned long long sums[4], unsigned long long* dropped);

// One pass of an extraction over the slots: VOXEL_W_OUT zeroed, the launch, the list's length; with n_tris, the same for the second
// list's word, VOXEL_W_TRIS.  h is entered and locked.
int voxel_pass(VoxelHost* h, const VoxelLaunch& launch, unsigned long long* n, unsigned long long* n_tris = nullptr);

// The count (list.count_only) or the sorted list of an extraction: a first pass for the number, a second one into a list of that size.
// launch(out, out_cap, stream) starts the kernel over the slots that lists the items (out == null: only counts them).  The list's
// order is the kind's `bool voxel_item_less(const Item&, const Item&)`, declared before the call (an overload, so that the sort
// inlines it).
template <class Item>
int voxel_extract(const char* where, VoxelRegistry& reg, const void* handle, uint32_t min, const VoxelList<Item>& list,
                  const std::function<void(Item* out, unsigned long long out_cap, hipStream_t)>& launch) {
    if (!voxel_known(reg, handle)) { viso_set_error("%s: not a live %s handle", where, reg.kind.handle); return VISO_ERR_ARG; }
    if (!list.n || min < 1 || (!list.count_only && list.cap && !list.out)) {
        viso_set_error("%s: bad argument (%s >= 1, non-null outputs)", where, reg.kind.threshold);
        return VISO_ERR_ARG;
    }
    VoxelSession ses(where, reg, handle);
    VISO_TRY(ses.status());
    unsigned long long c = 0, c2 = 0;
    VISO_TRY(voxel_pass(ses.host(), [&](hipStream_t s) { launch(nullptr, 0, s); }, &c));
    *list.n = (size_t)c;
    if (list.count_only || !c) return VISO_OK;
    if (c > list.cap) { viso_set_error("%s: %llu items do not fit the %zu given", where, c, list.cap); return VISO_ERR_ARG; }
    VoxelScratch d(ses, (size_t)c * sizeof(Item), "the list");
    VISO_TRY(d.status());
    VISO_TRY(voxel_pass(ses.host(), [&](hipStream_t s) { launch(d.as<Item>(), c, s); }, &c2));
    HIP_TRY(hipMemcpy(list.out, d.as<Item>(), (size_t)c * sizeof(Item), hipMemcpyDeviceToHost));
    VISO_TRY(d.release());   // (before the sort, not behind it)
    if (c2 != c) { viso_set_error("%s: the table changed between the two passes", where); return VISO_ERR_HIP; }   // (the map's lock rules it out)
    std::sort(list.out, list.out + c, [](const Item& x, const Item& y) { return voxel_item_less(x, y); });
    return VISO_OK;
}

// The count (list.count_only) or the sorted list of the voxels whose threshold word is at least `min`, as the payload p packs them:
// viso_*_count / viso_*_get, whole.  (p is the caller's own copy: the handle is not touched before the registry has answered.)
template <class P>
int voxel_entries(const char* where, VoxelRegistry& reg, const void* handle, uint32_t min, const VoxelList<typename P::Entry>& list, const P& p) {
    return voxel_extract<typename P::Entry>(where, reg, handle, min, list,
                                            [p, min](typename P::Entry* out, unsigned long long out_cap, hipStream_t s) {
        hipLaunchKernelGGL(voxel_compact_kernel<P>, dim3((p.head().mask + 1u) / 256u), dim3(256), 0, s, p, min, out, out_cap);
    });
}

// ---- eviction (include/viso_hip.h, "Map eviction"; the kernels are voxel_hash.h's) --------------------------------------------------
// the checks of an eviction's arguments that need no device; false: the error text is set
bool voxel_evict_args(const char* where, VoxelRegistry& reg, const void* handle, const viso_voxel_box* keep, const size_t* n);
// The statistics of h (entered and locked) as they lie on the device, [VOXEL_STAT_SETS][VOXEL_STAT_WORDS], and the sum of their
// occupied counters; voxel_evict_put_stats: the same block back with `less` fewer occupied slots, every other counter as it was.
int voxel_evict_get_stats(VoxelHost* h, std::vector<unsigned long long>& stats, unsigned long long* occupied);
int voxel_evict_put_stats(VoxelHost* h, std::vector<unsigned long long>& stats, unsigned long long less);
unsigned long long voxel_stat_sum(const std::vector<unsigned long long>& stats, int which);   // counter VOXEL_ST_`which` over the sets

// The second half of every call that takes voxels out of a table (an eviction, a retract): behind it no tombstone is left and every
// survivor is where a probe finds it.  A table with an empty slot: the leaving voxels' keys are tombstones by now; the rebuild pass
// moves every survivor up, the sweep empties the tombstones.  A table without one (`full`) has no cluster head to start a rebuild
// from: d_keep[n_keep] lists its survivors, and it goes through the clear and add_entries.  Either way the statistics `stats`, as
// voxel_evict_get_stats read them, go back with `less` fewer occupied slots.  h is entered and locked; the caller waits for the
// stream before `stats` and d_keep go.
template <class P>
int voxel_finish_removal(VoxelHost* h, const P& p, bool full, const typename P::Entry* d_keep, unsigned long long n_keep,
                         std::vector<unsigned long long>& stats, unsigned long long less) {
    hipStream_t s = h->ctx->stream;
    if (!full) {
        const dim3 grid((h->head.mask + 1u) / 256u);
        hipLaunchKernelGGL(voxel_evict_rebuild_kernel<P>, grid, dim3(256), 0, s, h->head, p);
        hipLaunchKernelGGL(voxel_evict_sweep_kernel<P>, grid, dim3(256), 0, s, h->head, p);
    } else {
        voxel_start_clear(p, s);
        if (n_keep) voxel_start_add_entries(p, d_keep, n_keep, s);
    }
    HIP_TRY(hipGetLastError());
    return voxel_evict_put_stats(h, stats, less);
}

// viso_*_evict_count (list.count_only) and viso_*_evict, whole.  A first pass counts the voxels outside the box; a second one lists them
// (list.out null: lists nothing) and turns their keys into tombstones, the rebuild pass moves every survivor to where a probe
// finds it, the sweep empties the tombstones; the occupied counter falls on the host.  Device memory: the list of the evicted.  A
// table without an empty slot has no cluster head to start a rebuild from: it goes through a list of its survivors, the clear
// and add_entries, and gets its statistics back.  The list's order is the kind's voxel_item_less, as in voxel_extract.
template <class P>
int voxel_evict(const char* where, VoxelRegistry& reg, const void* handle, const viso_voxel_box* keep, const VoxelList<typename P::Entry>& list,
                const P& p) {
    using Item = typename P::Entry;
    if (!voxel_evict_args(where, reg, handle, keep, list.n)) return VISO_ERR_ARG;
    VoxelSession ses(where, reg, handle);
    VISO_TRY(ses.status());
    VoxelHost* h = ses.host();
    VoxelBox box;
    for (int i = 0; i < 3; ++i) { box.lo[i] = keep->lo[i]; box.hi[i] = keep->hi[i]; }
    const size_t slots = (size_t)h->head.mask + 1;
    const dim3 grid((unsigned)(slots / 256));
    const VoxelTable head = h->head;
    auto mark = [&](int mode, Item* out, unsigned long long cap) {
        return [&, mode, out, cap](hipStream_t s) {
            hipLaunchKernelGGL(voxel_evict_mark_kernel<P>, grid, dim3(256), 0, s, head, p, box, mode, out, cap);
        };
    };
    unsigned long long c = 0, c2 = 0, occupied = 0;
    VISO_TRY(voxel_pass(h, mark(VOXEL_EVICT_COUNT, nullptr, 0), &c));
    *list.n = (size_t)c;
    if (list.count_only || !c) return VISO_OK;
    if (list.out && c > list.cap) { viso_set_error("%s: %llu items do not fit the %zu given", where, c, list.cap); return VISO_ERR_ARG; }
    std::vector<unsigned long long> stats;   // (before the block: the copy that puts them back reads them until its wait)
    VISO_TRY(voxel_evict_get_stats(h, stats, &occupied));
    const bool full = occupied >= slots;
    const unsigned long long n_keep = full ? slots - c : 0;
    const size_t b_out = list.out ? (size_t)c * sizeof(Item) : 0, b_keep = (size_t)n_keep * sizeof(Item);
    VoxelScratch d(ses, b_out + b_keep, "the list");   // the evicted | a full table's survivors
    VISO_TRY(d.status());
    Item* d_out = list.out ? d.as<Item>() : nullptr;
    Item* d_keep = d.as<Item>(b_out);
    hipStream_t s = ses.stream();
    if (!full) {
        VISO_TRY(voxel_pass(h, mark(VOXEL_EVICT_LIST, d_out, c), &c2));   // tombstones are in the table: voxel_finish_removal follows
    } else {
        if (d_out) VISO_TRY(voxel_pass(h, mark(VOXEL_EVICT_PEEK, d_out, c), &c2));
        else c2 = c;
        unsigned long long k2 = 0;
        if (n_keep) VISO_TRY(voxel_pass(h, mark(VOXEL_EVICT_KEEP, d_keep, n_keep), &k2));
        if (k2 != n_keep) c2 = ~0ull;
    }
    if (!full || c2 == c) VISO_TRY(voxel_finish_removal(h, p, full, d_keep, n_keep, stats, c2));
    if (d_out) HIP_TRY(hipMemcpyAsync(list.out, d_out, b_out, hipMemcpyDeviceToHost, s));
    VISO_TRY(d.release());
    if (c2 != c) { viso_set_error("%s: the table changed between the two passes", where); return VISO_ERR_HIP; }   // (the map's lock rules it out)
    if (list.out) std::sort(list.out, list.out + c, [](const Item& x, const Item& y) { return voxel_item_less(x, y); });
    return VISO_OK;
}

// ---- retract (include/viso_hip.h, "TSDF retract"; the check and the mark are voxel_hash.h's, the take is the kind's) --------------------
// the six words of the public report, in its order
struct VoxelRetractReport { unsigned long long n_points, n_updates, n_missing, n_underflow, n_inconsistent, n_freed; };
// The kind's launches over a group of frames: the take (the fuse's updates subtracted, through read-only probes; what it cannot
// place and what it takes below zero to VOXEL_W_MISSING and VOXEL_W_UNDERFLOW), the same with the sign flipped, and the fuse itself
// for a move.  bound: what the kind's payload compares with in P::within.
struct VoxelRetractLaunches { VoxelFuseLaunch take, undo, fuse; long long bound; };

// viso_*_retract and viso_*_move, whole, over the view v of the frames as they were fused; move: they are then fused again at
// poses_new ([v.n][16], or null for none), under the same session.  What voxel_fuse checks, in its order; then the take, the
// check over the slots, and either the commit (the freed slots leave the table as an eviction's do: voxel_finish_removal) or the
// undo, which leaves every word of the table as it was and returns VISO_ERR_ARG.  *report (or null) is filled either way.
template <class P>
int voxel_retract(const char* where, VoxelRegistry& reg, const void* handle, const DispView& v, bool move, const double* poses_new,
                  const VoxelRetractLaunches& L, const P& p, unsigned long long* report) {
    using Item = typename P::Entry;
    DispView v2 = v;
    v2.poses = poses_new;
    VISO_TRY(voxel_fuse_args(where, reg, handle, v));
    if (move) VISO_TRY(voxel_fuse_args(where, reg, handle, v2));
    VoxelSession ses(where, reg, handle, VoxelSession::ANY_STATE);   // the overflow refusal comes behind the context's
    VISO_TRY(ses.status());
    VoxelHost* h = ses.host();
    hipStream_t s = ses.stream();
    VoxelFrames f;
    VISO_TRY(voxel_fuse_stage(ses, reg, v, &f));
    const size_t slots = (size_t)h->head.mask + 1;
    const dim3 grid((unsigned)(slots / 256));
    const VoxelTable head = h->head;
    const long long bound = L.bound;
    // the take: the three counters fall on the device, what they fell by is the report's
    std::vector<unsigned long long> before, stats;   // (before the block: the copy that puts them back reads them until its wait)
    unsigned long long occupied = 0, words[2] = {0, 0};
    static_assert(VOXEL_W_UNDERFLOW == VOXEL_W_MISSING + 1, "the two words of a retract are read as one");
    HIP_TRY(hipMemsetAsync(h->head.words + VOXEL_W_MISSING, 0, sizeof(words), s));
    VISO_TRY(voxel_evict_get_stats(h, before, &occupied));
    VISO_TRY(voxel_fuse_groups(h, v, f, L.take));
    // the check, behind the take on the stream: its two counts run on in the sets, like the counters
    hipLaunchKernelGGL(voxel_retract_check_kernel<P>, grid, dim3(256), 0, s, head, p, bound);
    HIP_TRY(hipGetLastError());
    VISO_TRY(voxel_evict_get_stats(h, stats, &occupied));
    VISO_TRY(voxel_read_words(h, VOXEL_W_MISSING, 2, words));
    VoxelRetractReport rep{};
    rep.n_points = voxel_stat_sum(before, VOXEL_ST_POINTS) - voxel_stat_sum(stats, VOXEL_ST_POINTS);
    rep.n_updates = voxel_stat_sum(before, VOXEL_ST_UPDATES) - voxel_stat_sum(stats, VOXEL_ST_UPDATES);
    rep.n_freed = voxel_stat_sum(stats, VOXEL_ST_FREED) - voxel_stat_sum(before, VOXEL_ST_FREED);
    rep.n_inconsistent = voxel_stat_sum(stats, VOXEL_ST_BAD) - voxel_stat_sum(before, VOXEL_ST_BAD);
    rep.n_missing = words[0]; rep.n_underflow = words[1];
    static_assert(sizeof(rep) == 6 * sizeof(unsigned long long), "the report is six words");
    if (report) std::copy(&rep.n_points, &rep.n_points + 6, report);
    if (rep.n_missing || rep.n_underflow || rep.n_inconsistent) {
        // the undo: the same launches find the same slots (no key was written), and the modular adds restore every word
        VISO_TRY(voxel_fuse_groups(h, v, f, L.undo));
        HIP_TRY(hipStreamSynchronize(s));
        viso_set_error("%s: these are not frames of this %s as they were fused: n_missing %llu (updates whose voxel is not in the table), "
                       "n_underflow %llu (not zero: a weight fell below zero), n_inconsistent %llu (voxels left beyond their bounds); the %s is unchanged",
                       where, reg.kind.noun, rep.n_missing, rep.n_underflow, rep.n_inconsistent, reg.kind.noun);
        return VISO_ERR_ARG;
    }
    if (rep.n_freed) {
        const bool full = occupied >= slots;
        const unsigned long long n_keep = full ? slots - rep.n_freed : 0;
        VoxelScratch d(ses, (size_t)n_keep * sizeof(Item), "the list");   // a full table's survivors
        VISO_TRY(d.status());
        unsigned long long c2 = rep.n_freed;
        if (!full) {
            hipLaunchKernelGGL(voxel_retract_mark_kernel<P>, grid, dim3(256), 0, s, head, p, bound);   // tombstones are in the table:
            HIP_TRY(hipGetLastError());                                                                // voxel_finish_removal follows
        } else if (n_keep) {
            unsigned long long k2 = 0;   // the survivors are the slots of threshold word >= 1: the getters' list
            VISO_TRY(voxel_pass(h, [&](hipStream_t st) {
                hipLaunchKernelGGL(voxel_compact_kernel<P>, grid, dim3(256), 0, st, p, 1u, d.as<Item>(), n_keep);
            }, &k2));
            if (k2 != n_keep) c2 = ~0ull;
        }
        if (!full || c2 == rep.n_freed) VISO_TRY(voxel_finish_removal(h, p, full, d.as<Item>(), n_keep, stats, c2));
        VISO_TRY(d.release());
        if (c2 != rep.n_freed) { viso_set_error("%s: the table changed between the two passes", where); return VISO_ERR_HIP; }   // (the map's lock rules it out)
    }
    if (!move) return VISO_OK;
    VISO_TRY(voxel_fuse_restage(ses, poses_new, v.n, &f));
    VISO_TRY(voxel_fuse_groups(h, v2, f, L.fuse));
    return voxel_finish(where, h);
}
#endif /* VISO_VOXEL_HOST_H_ */
