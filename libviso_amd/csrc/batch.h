// batch.h — private to the three batch files: struct viso_batch, the helpers every part needs, and the functions that cross them.
//   batch.hip             create / destroy / free, item builders, uploads (rectify with them), detect, set_params, the run itself
//                         (matcher, sub-pixel, circle join, RANSAC), the core getters, timing and stamps
//   batch_dense.hip       the dense maps of the resident images: block matching, SGM, speckle, points, the voxel fuse
//   batch_estimators.hip  the opt-in estimators behind the RANSAC stage: covariance, refine, window
//
// HBM layout (allocated at viso_batch_create unless an opt-in stage is named):
//   kp      [nf][2][cap] float2          boundary layout (x,y)
//   desc    [nf][2][cap][dlen] float     boundary layout (reference Mat N x 121 CV_32F)
//   packed  [nf][2][cap][128] u16        biased rows the matcher reads (256 B, 16-B aligned)
//   res     [3][nf][cap] int2            per query (target | -1, SAD)
//   sorted  [3][nf][cap][3] int          match lists in (dist,i1) order; pos = inverse
//   x_c [nf][4][cap], Xp_c [nf][3][cap]   double, SoA rows like cv::Mat(4,M): the solver's inputs, written by the circle join
//   uv  [nf][cap] float2                 refined right-image points per stereo row (viso_batch_set_subpixel != 0 only)
//   raw [nf][2][raw_rows][raw_cols] u8   staged raw images the remap reads into `images` (viso_batch_set_rectify only)
//   disp [nf][img_rows][img_cols] i16    dense disparity of every frame's resident pair (viso_batch_set_disparity / _set_sgm only)
//   sgm_ws                               census words and S volumes of one group of frames (viso_batch_set_sgm only; sgm.hip)
//   spk_ws                               label and size words of one group of frames (viso_batch_set_speckle only; speckle.hip)
// `which` = 0 stereo L->R of frame t, 1 temporal left (t vs t-1), 2 temporal right.
#pragma once
#include "common.h"

#include <string.h>
#include <initializer_list>
#include <vector>

#define VISO_NPIN_SLOTS 4
#define VISO_EVENT_POOL 64

// One buffer of viso_batch::alloc_zeroed: the pointer to set and its size.
struct DBuf {
    void** p; size_t bytes;
    template <class T> DBuf(T** q, size_t count) : p(reinterpret_cast<void**>(q)), bytes(sizeof(T) * (count ? count : 1)) {}
};

// Opt-in rectification of raw images (rectify.hip): on while map != null; the quantised maps [2][img_rows * img_cols], the raw
// staging buffer, its geometry and the border value
struct BatchRectify { RectEntry* map = nullptr; uint8_t* raw = nullptr; int raw_rows = 0, raw_cols = 0, border = 0; size_t raw_bytes = 0; };

struct BatchDense {
    // opt-in dense disparity (disparity.hip): on while disp_on; the parameters, the maps (allocated when first needed, for the
    // geometry rows x cols), and whether the maps hold the last image geometry's result (0: no run has computed them)
    bool disp_on = false; viso_disparity_params disp_p = {}; int16_t* disp = nullptr; size_t disp_bytes = 0; int rows = 0, cols = 0; int last = 0;
    // opt-in semi-global matching (sgm.hip): on while sgm_on (never together with disp_on: the maps are one buffer, `disp`); the
    // parameters and the workspace of one group of frames (allocated by the first launch, again when a launch needs another size)
    bool sgm_on = false; viso_sgm_params sgm_p = {}; void* sgm_ws = nullptr; size_t sgm_ws_bytes = 0;
    // opt-in speckle filter of the maps (speckle.hip): on while spk_on, behind either method's selection kernel; the parameters and
    // the workspace of one group of frames (allocated by the first launch, again when a launch needs another size)
    bool spk_on = false; viso_speckle_params spk_p = {}; void* spk_ws = nullptr; size_t spk_ws_bytes = 0;
    bool on() const { return disp_on || sgm_on; }
    bool speckle() const { return spk_on && spk_p.max_size > 0; }
};

// What the three opt-in estimators share: the mode and sigma asked for, the records [nf] (allocated on the first request, frame 0
// stays zero: status 0), and what the last run computed them with (0: the last run computed none)
template <class Rec> struct BatchRecords { int mode = 0; double sigma = 0.0; Rec* rec = nullptr; int last = 0; };

struct BatchEstimators {
    BatchRecords<viso_motion_cov> cov;      // opt-in motion covariance (covariance.hip)
    // opt-in motion refinement (refine.hip): the working buffers are points [nf][2][3][cap] and L' [nf][cap]
    BatchRecords<viso_motion_refine> ref; double* ref_pts = nullptr; int* ref_idx = nullptr;
    // opt-in window refinement (window.hip): K (0 off; win.last is the K of the last run) and the working buffers (L' [nf][cap],
    // |L'| [nf], tables [nf][2][cap], tracks [nf][5][(K-1) cap], points [nf][2][3][(K-1) cap]; allocated on the first request with
    // K > 0, for the largest K asked for so far: win_kalloc)
    BatchRecords<viso_window_record> win; int win_K = 0, win_kalloc = 0;
    int *win_lp = nullptr, *win_nlp = nullptr, *win_tab = nullptr, *win_trk = nullptr; double* win_pts = nullptr;
};

struct viso_batch {
    viso_ctx* ctx = nullptr;
    int nf = 0, cap = 0, dlen = 0, iters = 0;
    int n_probs = 0;           // padded problem count (multiple of 24)
    // Every device buffer the batch owns, recorded when it is allocated: the addresses of the pointer members that alloc,
    // alloc_zeroed and fit filled.  viso_batch_free walks the record; release frees one buffer early.  ovf_cnt, bad_img, bad_any, ok
    // and n_inl are views into the blocks of scored and tr, not buffers of their own: they are never recorded.
    std::vector<void**> owned;
    void own(void** p);   // records p once
    int alloc_bytes(void** p, size_t bytes);
    template <class T> int alloc(T** p, size_t count) { return alloc_bytes(reinterpret_cast<void**>(p), sizeof(T) * count); }
    // every buffer of the list, zeroed; when an allocation fails, the buffers already allocated are freed and every pointer is null
    int alloc_zeroed(std::initializer_list<DBuf> bufs);
    int release_bytes(void** p);
    template <class T> int release(T** p) { return release_bytes(reinterpret_cast<void**>(p)); }
    // *p holds `want` bytes afterwards (*have follows): kept when it already does (grow_only: or more), else replaced after the
    // batch's work in flight.  When the allocation fails *p is null and the sticky HIP error cleared; `what` names the buffer in a
    // VISO_ERR_NOMEM message for `where`, null reports the HIP error.
    int fit_bytes(void** p, size_t* have, size_t want, bool grow_only, const char* where, const char* what);
    template <class T> int fit(T** p, size_t* have, size_t want, bool grow_only = false, const char* where = nullptr, const char* what = nullptr) {
        return fit_bytes(reinterpret_cast<void**>(p), have, want, grow_only, where, what);
    }

    float2* kp = nullptr; float* desc = nullptr; int* n = nullptr; uint16_t* packed = nullptr; uint8_t* packed8 = nullptr; uint2* sums = nullptr;
    // the 8-bit planes' shift (VISO_R8_*, csrc/common.h): device counters, their pinned landing place, the event behind the copy
    int* r8cnt = nullptr; int* r8pin = nullptr; hipEvent_t r8ev = nullptr; bool r8pending = false; int r8shift = VISO_R8_DEFAULT; int r8last = VISO_R8_DEFAULT; unsigned r8runs = 0;
    int* bad_img = nullptr; int* bad_any = nullptr; int* zero = nullptr;
    float2* skp = nullptr; int *sidx = nullptr, *rank = nullptr, *bstart = nullptr; float* xinfo = nullptr; uint8_t* qord = nullptr;   // column-bucket view of every image
    uint8_t* images = nullptr; int img_rows = 0, img_cols = 0;   // optional: [nf][2][rows][cols] uint8 (image-in mode)
    float* h_resp = nullptr; float2* h_tmp_kp = nullptr; float* h_tmp_resp = nullptr; int* h_cnt = nullptr; size_t h_slots = 0;   // Harris detector scratch
    void* h_part = nullptr; size_t h_part_bytes = 0;                                                                          // ... of the strip kernel (harris_strip_bytes)
    ImageView* views = nullptr;                                  // [nf*2] (+1 empty)
    MatchProblem* probs = nullptr;
    int2* ovf_q = nullptr;                 // the launch's overflow queue: up to one entry per query of the batch
    int* tile_flag = nullptr; int tiles = 0;   // [3][nf][tiles] per-64-query-tile scratch of the stereo kernels
    int2* res = nullptr; int* sorted = nullptr; int* pos = nullptr; int* m_cnt = nullptr; int* ovf_cnt = nullptr; unsigned long long* scored = nullptr; size_t zeroed_bytes = 0;
    double *x_c = nullptr, *Xp_c = nullptr;   // the solver's inputs: gathered + triangulated by the circle join
    // opt-in sub-pixel refinement of the stereo observations (subpixel.hip): the mode asked for, the buffer (allocated on the first
    // request), and the mode the last run refined with (0: the last run produced no refined points)
    int subpix = 0; float2* uv = nullptr; int uv_mode = 0;
    BatchRectify rect;
    BatchDense dense;
    BatchEstimators est;
    JoinItem* join = nullptr; SolverItem* sitems = nullptr;
    int *circ = nullptr, *pcl = nullptr, *mc = nullptr;
    double* tr_h = nullptr; int *ok_h = nullptr, *cnt_h = nullptr, *hq = nullptr; char* rot = nullptr;   // hq: list of undecided hypotheses (launch_ransac)
    int* samp_h = nullptr;                  // [nf][iters][3] sample triples of the run (ransac_hyp_kernel)
    // the *_async uploads stage the caller's (pageable, possibly temporary) n array through a small pinned ring:
    // slot k is reusable once the copy that read it has passed (n_pin_ev[k])
    int* n_pin = nullptr; hipEvent_t n_pin_ev[VISO_NPIN_SLOTS] = {}; bool n_pin_used[VISO_NPIN_SLOTS] = {}; int n_pin_next = 0;
    double* tr = nullptr; int *ok = nullptr, *n_inl = nullptr, *inl = nullptr;   // tr, ok, n_inl: ONE device block (tr first), mirrored in pinned memory by every run's last kernel
    unsigned char* pose_pin = nullptr;   // [n_frames] x (6 doubles) | [n_frames] ok | [n_frames] n_inl: what viso_batch_get_poses reads
    size_t pose_bytes = 0;
    MatchParamsDev mp[2] = {};
    SolverParamsDev sp = {};
    unsigned long long seed = 0, first_frame = 0;
    bool params_set = false;
    bool timing = false;
    bool desc_i16 = false;     // the descriptor buffer holds int16 rows (viso_batch_upload_i16*), not the f32 boundary layout
    std::vector<signed char> desc_family;   // per frame: 0 = never uploaded, 1 = f32 rows, 2 = int16 rows (the two must not mix in a run)
    // The RANSAC stage of run k (latency bound: a few hundred waves on serial fp64 chains for ~1 ms) runs on a
    // stream of its own (the context's second stream), so that the matcher of run k+1 — which touches none of its
    // buffers — fills the GPU beside it: stream (matcher, triangulation, circle join) --ev_join--> solver_stream (RANSAC) --ev_ransac--> the next
    // run's circle join (which rewrites the RANSAC inputs).
    hipStream_t solver_stream = nullptr;
    hipEvent_t ev_join = nullptr, ev_ransac = nullptr;
    bool ransac_pending = false;
    // matcher-kernel timing: event pairs of the runs not yet read back (bounded: the oldest pair is folded into
    // the running sum and reused once VISO_EVENT_POOL pairs are outstanding)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t ev_next = 0;        // ring position of the oldest outstanding pair
    double ev_ms_sum = 0; int ev_n = 0;
    // viso_batch_stamp: time stamps of a run (0 = before its uploads, 1 = after them, 2 = behind its last kernel)
    hipEvent_t ev_stamp[3] = {};
    bool stamps = false;
    // loop closure (loops.hip): a matcher launch has filled the packed rows, and the workspace of its batch calls (grow only)
    bool has_run = false; char* loop_ws = nullptr; size_t loop_ws_bytes = 0;
};

// A handle the library does not know -- null, destroyed, or taken along by viso_ctx_destroy of its context (ctx.hip keeps the
// registry): every entry point answers VISO_ERR_ARG instead of following a freed pointer.
static inline bool dead(const viso_batch* b) { return !b || !viso_batch_live(b); }

static inline int enter(viso_batch* b) {   // every entry point that allocates, copies or launches
    HIP_TRY(hipSetDevice(b->ctx->device));
    return VISO_OK;
}

static inline int batch_sync(viso_batch* b) {   // everything the batch has in flight: matcher stream, then its RANSAC stream
    HIP_TRY(hipStreamSynchronize(b->ctx->stream));
    if (b->solver_stream) HIP_TRY(hipStreamSynchronize(b->solver_stream));
    return VISO_OK;
}

static inline bool slot_ok(viso_batch* b, int which, int t) { return !dead(b) && which >= 0 && which < 3 && t >= 0 && t < b->nf; }
static inline int prob_slot(int which, int t) { return (t / 8) * 24 + which * 8 + (t % 8); }
// the batch's resident images, frames f0 .. f0+n-1, as every launcher takes them (common.h)
static inline StereoImages batch_images(const viso_batch* b, int f0, int n) { return image_block(b->images, b->img_rows, b->img_cols, f0, n); }

// batch_dense.hip, for viso_batch_run_images (which has entered the device): the limits a dense launch over the resident images
// must respect, then the launch itself on the context's stream; errors name `where`
int dense_preflight(viso_batch* b, const char* where);
int launch_batch_disparity(viso_batch* b, const char* where);
// batch_estimators.hip, for run_rest: the opt-in estimators that are on, on the solver's stream ss behind the RANSAC stage
int batch_launch_estimators(viso_batch* b, hipStream_t ss);
