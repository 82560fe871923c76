// voxel_host.h — the host side of the shared table layer of the hash tables of voxels (voxelmap.hip, tsdf.hip; the device side is
// voxel_hash.h; DESIGN.md 5.14, "Shared table layer").  A kind of map (viso_map, viso_tsdf) holds a VoxelHost, has a VoxelRegistry
// of its live handles, and passes its kernel launches in as callables.  The rules that every kind must keep are here and in
// voxel_host.hip, once: no handle is dereferenced before its registry has answered for it; staging is freed only behind a
// synchronise; dropped updates become the sticky overflow mark; a temporary list is freed on every path.
#ifndef VISO_VOXEL_HOST_H_
#define VISO_VOXEL_HOST_H_
#include "voxel_hash.h"

#include <algorithm>
#include <functional>
#include <mutex>
#include <unordered_map>

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
// one group of views; d_gray: the group's part of the third output, or null when the call has none
using VoxelRenderLaunch = std::function<void(const double* d_poses, int16_t* d_disp, uint32_t* d_weight, uint8_t* d_gray, dim3 grid, hipStream_t)>;
// one group of frames of a linearise: the group's poses [.][12], its flags and its part of the sums, the group's first frame
using VoxelLinearizeLaunch = std::function<void(const double* d_poses, const unsigned long long* d_active, unsigned long long* d_out, int frame0,
                                                dim3 grid, hipStream_t)>;
using VoxelEntriesLaunch = std::function<void(const void* d_entries, dim3 grid, hipStream_t)>;   // add_entries

bool voxel_known(VoxelRegistry& reg, const void* handle);
// a live handle whose context is alive, its device current: *h set; else the error text and code
int voxel_enter(const char* where, VoxelRegistry& reg, const void* handle, VoxelHost** h);
int voxel_refuse_overflowed(const char* where, const VoxelHost* h);

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

// map_fuse_resident / tsdf_fuse_resident (common.h) and viso_*_fuse, whole: the handle and argument checks, the staging of the
// poses and of the host map, the groups of frames, each started by `launch`, and the wait that finds a full table.  image (or
// null): frame f's 8-bit image at image + f * ifs on the device (resident), or one host image of the map's size that is staged like
// the map (host); each group's launch is handed its first image.
int voxel_fuse_resident(const char* where, VoxelRegistry& reg, const void* handle, viso_ctx* c, const int16_t* disp, size_t mfs, int rows,
                        int cols, int n_frames, double f, double cu, double cv, double base, const double* poses, const VoxelFuseLaunch& launch,
                        const uint8_t* image = nullptr, size_t ifs = 0);
int voxel_fuse_host(const char* where, VoxelRegistry& reg, const void* handle, const int16_t* disp, int rows, int cols, const viso_param* param,
                    const double* pose_or_null, const VoxelFuseLaunch& launch, const uint8_t* image = nullptr);
// viso_*_add_entries behind the handle check and the validation of the n entries of entry_bytes each
int voxel_add_entries(const char* where, VoxelRegistry& reg, const void* handle, const void* entries, size_t n, size_t entry_bytes,
                      const VoxelEntriesLaunch& launch);
// viso_*_render behind the handle and argument checks: the map entered, locked and not overflowed; the poses [n_views][16] (or
// null) through d_pose; a device buffer for n_views maps of px int16 and, with weight_out, as many uint32, and, with gray_out, as
// many uint8, freed on every path; the groups of views, each started by `launch` with its poses ([.][12] or null) and its part of
// the buffer; the copies to the host.
int voxel_render(const char* where, VoxelRegistry& reg, const void* handle, size_t px, const double* poses, int n_views, int16_t* disp_out,
                 uint32_t* weight_out, const VoxelRenderLaunch& launch, uint8_t* gray_out = nullptr);
// A host map of px pixels into the fuse's staging d_disp (grow-only), on the stream; *d_disp: where it is.  h is entered and locked.
int voxel_stage_map(const char* where, VoxelHost* h, const int16_t* disp, size_t px, const int16_t** d_disp);
// One linearise of an alignment (include/viso_hip.h, "TSDF align") for n frames: h is entered, locked and not overflowed (the
// caller holds the lock over the whole alignment).  The poses [n][16] as [n][12], the flags active [n] (0: the frame's lanes
// leave at once) and `words` zeroed 64-bit sums a frame go through d_pose (grow-only), the groups of frames are started by `launch`
// with blocks_x blocks along x, and the sums come back to out [n][words].
int voxel_linearize(const char* where, VoxelHost* h, const double* poses, const unsigned long long* active, int n, size_t words,
                    unsigned blocks_x, unsigned long long* out, const VoxelLinearizeLaunch& launch);
// viso_*_stats: the four counters summed over the sets (VOXEL_ST_*) and the dropped word
int voxel_stats(const char* where, VoxelRegistry& reg, const void* handle, const void* out, unsigned long long sums[4], unsigned long long* dropped);

// One pass of an extraction over the slots: VOXEL_W_OUT zeroed, the launch, the list's length.  h is entered and locked.
int voxel_pass(VoxelHost* h, const VoxelLaunch& launch, unsigned long long* n);

// The count (count_only) or the sorted list of an extraction: a first pass for the number, a second one into a list of that size.
// launch(out, out_cap, stream) starts the kernel over the slots that lists the items (out == null: only counts them).  The list's
// order is the kind's `bool voxel_item_less(const Item&, const Item&)`, declared before the call (an overload, so that the sort
// inlines it).
template <class Item>
int voxel_extract(const char* where, VoxelRegistry& reg, const void* handle, uint32_t min, bool count_only, Item* items_out, size_t n_cap,
                  size_t* n, const std::function<void(Item* out, unsigned long long out_cap, hipStream_t)>& launch) {
    if (!voxel_known(reg, handle)) { viso_set_error("%s: not a live %s handle", where, reg.kind.handle); return VISO_ERR_ARG; }
    if (!n || min < 1 || (!count_only && n_cap && !items_out)) {
        viso_set_error("%s: bad argument (%s >= 1, non-null outputs)", where, reg.kind.threshold);
        return VISO_ERR_ARG;
    }
    int r;
    VoxelHost* h;
    if ((r = voxel_enter(where, reg, handle, &h)) < 0) return r;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->overflowed) return voxel_refuse_overflowed(where, h);
    unsigned long long c = 0, c2 = 0;
    if ((r = voxel_pass(h, [&](hipStream_t s) { launch(nullptr, 0, s); }, &c)) < 0) return r;
    *n = (size_t)c;
    if (count_only || !c) return VISO_OK;
    if (c > n_cap) { viso_set_error("%s: %llu items do not fit the %zu given", where, c, n_cap); return VISO_ERR_ARG; }
    Item* d = nullptr;
    if (hipMalloc((void**)&d, (size_t)c * sizeof(Item)) != hipSuccess) {
        (void)hipGetLastError();
        viso_set_error("%s: cannot allocate %zu bytes for the list", where, (size_t)c * sizeof(Item));
        return VISO_ERR_NOMEM;
    }
    r = voxel_pass(h, [&](hipStream_t s) { launch(d, c, s); }, &c2);
    hipError_t e = hipSuccess;
    if (r >= 0) e = hipMemcpy(items_out, d, (size_t)c * sizeof(Item), hipMemcpyDeviceToHost);
    (void)hipFree(d);   // on every path
    if (r < 0) return r;
    HIP_TRY(e);
    if (c2 != c) { viso_set_error("%s: the table changed between the two passes", where); return VISO_ERR_HIP; }   // (the map's lock rules it out)
    std::sort(items_out, items_out + c, [](const Item& x, const Item& y) { return voxel_item_less(x, y); });
    return VISO_OK;
}
#endif /* VISO_VOXEL_HOST_H_ */
