/*
 * viso_hip.h — C-ABI of libviso_hip.so, the MI355X (gfx950) implementation of
 * libviso's per-frame hot path: descriptor-window SAD matcher, circular-match
 * join, rectified triangulation and the RANSAC + Gauss-Newton stereo
 * reprojection pose solver.
 *
 * Every entry point replaces one free function of the reference
 * (alexkreimer/libviso, paths relative to its root); the reference has no FFI
 * of its own (plain C++ free functions over cv::Mat / std::vector), so this
 * header is what a cgo/ctypes/C++ adapter binds instead.  INTEGRATION.md shows
 * the reference-side adapter.
 *
 * Conventions
 *   - plain pointers and sizes only; all matrices are row-major and contiguous;
 *   - "4xM" / "3xM" double matrices are SoA exactly like the reference's
 *     cv::Mat(4,M,CV_64F): row r starts at p + r*M;
 *   - return value: 1 = true, 0 = false (the reference's bool), negative =
 *     VISO_ERR_* (the reference would assert/abort; we never abort across the ABI);
 *   - the *_dev / batch family takes DEVICE pointers and a context (persistent
 *     device buffers + one HIP stream); the plain family takes HOST pointers and
 *     runs on a lazily created default context.
 *   - nothing here computes on the CPU: if the HIP device is missing the calls
 *     fail with VISO_ERR_HIP.
 */
#ifndef VISO_HIP_H_
#define VISO_HIP_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VISO_OK 1
#define VISO_FALSE 0
#define VISO_ERR_ARG (-1)         /* bad argument (the reference asserts: src/viso.cpp:676,174-175) */
#define VISO_ERR_HIP (-2)         /* HIP runtime error / no device */
#define VISO_ERR_UNSUPPORTED (-3) /* size beyond what this build handles */
#define VISO_ERR_NOMEM (-4)

#define VISO_DESC_LEN 121 /* (2*5+1)^2, src/viso.cpp:1001,1174 */

/* Mirrors `struct MatchParams` (src/viso.cpp:48-75).  `alg_thresh` and
 * `allow_ann` are never read by match_desc and are omitted. */
typedef struct viso_match_params {
    int32_t enforce_epipolar;   /* src/viso.cpp:50 */
    int32_t enforce_2nd_best;   /* :55 */
    int32_t max_neighbors;      /* :59  K, columns of the neighbour matrix */
    int32_t _pad;
    double F[9];                /* :51  row-major fundamental matrix, x2' F x1 = 0 */
    double sampson_thresh;      /* :53 */
    double ratio_2nd_best;      /* :56 */
    double radius;              /* :60  L1 pixel radius (cast to float at :685) */
} viso_match_params;

/* Mirrors `struct param` (src/viso.h:58-72). */
typedef struct viso_param {
    double base;                /* :61 */
    int32_t ransac_iter;        /* :62 default 50 */
    int32_t save_debug;         /* :65 unused by the hot path, kept for layout parity */
    double inlier_threshold;    /* :63 default 2 */
    double thresh;              /* :64 default 1e-4 */
    double f, cu, cv;           /* :66-71 calib.{f,cu,cv} */
} viso_param;

/* MatchParams(F) ctor, src/viso.cpp:62-71: stereo L->R (epipolar on, K=200, r=80). */
void viso_match_params_stereo(viso_match_params* mp, const double F[9]);
/* MatchParams() ctor, src/viso.cpp:72-74: temporal (2nd-best 0.9, K=250, r=80). */
void viso_match_params_temporal(viso_match_params* mp);
/* param() ctor, src/viso.h:60. base/f/cu/cv are left 0. */
void viso_param_default(viso_param* p);

/* ---------------------------------------------------------------- context */
typedef struct viso_ctx viso_ctx;

/* device: HIP device ordinal.  stream: a hipStream_t to run on, or NULL to let
 * the context create its own.  Returns NULL on failure (viso_last_error()). */
viso_ctx* viso_ctx_create(int device, void* stream);
/* Waits for the streams, frees the context.  VISO_OK, or VISO_ERR_HIP with the first HIP error met in
 * viso_last_error() (everything that can be freed still is).  Batches of the context that are still alive are destroyed
 * with it, FIRST (the library keeps a registry of its live handles): the intended order is batches, then context, but the
 * other order costs nothing worse than a return code -- a later viso_batch_destroy of such a batch is a no-op (VISO_OK, once),
 * every other call on it returns VISO_ERR_ARG, and so does anything on a context or batch handle that was destroyed before
 * or never existed.  Destroy handles before the process starts exiting: not from static destructors that may run after the
 * HIP runtime's own. */
int viso_ctx_destroy(viso_ctx* ctx);
/* hipStream_t the context launches on.  Every context also owns a second stream for the RANSAC
 * stage of its batches (it runs beside the next run's matcher; ordered by events, waited for by
 * viso_ctx_synchronize and by every getter): a host that orders its own work against viso_ctx_stream() must
 * use viso_ctx_synchronize (or a result getter) to see poses, not a bare hipStreamSynchronize of that stream. */
void* viso_ctx_stream(viso_ctx* ctx);
int viso_ctx_synchronize(viso_ctx* ctx);
/* Which kernel takes the temporal match_desc calls of this context (ctx == NULL: the default context of the
 * plain family).  The product build offers three: 6 = match_union8_kernel (the default: a wave ranks every row of a
 * round's union list against eight y-adjacent queries on the rows' 8-bit planes, scores the two best candidates of a
 * query exactly, and lets a rigorous lower bound of the rest decide whether that settles match_desc),
 * 3 = match_union_kernel (the same round structure on the u16 rows: every pair scored exactly; the default until
 * round 4) and 5 = match_prune_kernel (exact successive elimination on block sums in front of a cell-granular scorer).
 * Further variants (2 = match_batch_kernel<0>, 4 = match_strip_kernel) exist in -DVISO_DEBUG_VARIANTS builds only.
 * Every variant gives identical results, and the parity tests run over whatever viso_matcher_variants() reports for
 * the build under test.  Returns VISO_ERR_ARG for a variant this build does not have. */
int viso_ctx_set_matcher(viso_ctx* ctx, int variant);
/* The variants of this build: fills out[0..cap), returns their number.  Needs no device. */
int viso_matcher_variants(int* out, int cap);
/* The variant a new context starts with: the build's default, or $VISO_MATCHER when that names a variant of this build
 * (an A/B and test aid).  Needs no device. */
int viso_matcher_default(void);
/* How the RANSAC stage splits the <= 100 Gauss-Newton iterations of a 3-point hypothesis (src/viso.cpp:1593) between
 * its two kernels: the lane-per-hypothesis kernel runs the first `split`, the wave-per-hypothesis kernel the rest of
 * the few that are still undecided.  0 = the build's default (10); 100 = the lane kernel alone.  Every split gives
 * bit-identical hypotheses (tests/test_gpu_solver_edges.py); this is a tuning / test knob.  ctx == NULL: the default
 * context of the plain family. */
int viso_ctx_set_gn_split(viso_ctx* ctx, int split);
/* match_union8_kernel (matcher variant 6) ranks candidates on 8-bit planes h(v) = clamp((v + (128 << s)) >> s, 0, 255) of the
 * descriptor rows.  shift = -1 (default): s is chosen per run from the descriptor magnitudes the previous run of the batch
 * packed (the smallest s that clamps at most one element pair in 256; 3 before any statistics exist and in the one-call
 * plain family); 0..3: fixed.  Every s gives the same results — the bound behind the ranking holds for any s and any
 * descriptors — it only decides how often the kernel has to score more than two candidates of a query exactly.
 * $VISO_ROW8_SHIFT sets the same for every new context (test / A-B aid). */
int viso_ctx_set_row8_shift(viso_ctx* ctx, int shift);
/* Name of that kernel as it appears in rocprofv3 summaries. */
const char* viso_ctx_matcher_kernel_name(viso_ctx* ctx);
const char* viso_last_error(void);
/* "libviso_hip <version> gfx950 ..." */
const char* viso_version(void);

/* ------------------------------------------------------ plain (host) family */

/* match_desc, src/viso.cpp:669-726 (+ radiusSearch :170-203, sampsonDistance
 * :655-666, kp2mat :246-256).  kp*: n x 2 float (x,y).  d*: n x dlen float.
 * out_match: up to n1 rows (i1,i2,(int)dist), sorted by (dist asc, i1 asc) —
 * the reference's std::sort is unstable (:724); this is the documented
 * tightening.  *out_n = number of matches. */
int viso_match_desc(const float* kp1, int n1, const float* kp2, int n2,
                    const float* d1, const float* d2, int dlen,
                    const viso_match_params* mp,
                    int32_t* out_match, int* out_n);

/* match_circle, src/viso.cpp:207-243.  Lists are n x 3 int32 (i1,i2,dist).
 * circ: up to cap x 4, pcl: up to cap x 2 (positions into lr / lr_prev).
 * Exact for arbitrary lists (duplicate keys included): output order is the
 * reference's nested-loop order.  Returns VISO_ERR_ARG if more than cap rows
 * would be produced (*out_n then holds the required count). */
int viso_match_circle(const int32_t* lr, int n_lr, const int32_t* lr_prev, int n_lrp,
                      const int32_t* m11, int n11, const int32_t* m22, int n22,
                      int32_t* circ, int32_t* pcl, int cap, int* out_n);

/* collect_matches(...,Mat& x) src/viso.cpp:501-514: x = 4 x n double
 * (uL,vL,uR,vR). */
int viso_collect_matches(const float* kp1, int n1, const float* kp2, int n2,
                         const int32_t* match, int n, double* x4xn);

/* triangulate_rectified<double>, src/viso.cpp:1137-1162. */
int viso_triangulate_rectified(const double* x4xM, int m, const viso_param* p,
                               double* X3xM);

/* minimize_reproj, src/viso.cpp:1583-1623.  tr is in/out.  1 = converged,
 * 0 = singular system or 100 iterations exhausted. */
int viso_minimize_reproj(const double* X3xM, const double* obs4xM, int m,
                         double tr[6], const viso_param* p,
                         const int32_t* active, int n_active);

/* get_inliers, src/viso.cpp:1509-1537.  inliers: up to m ascending indices.
 * rms (may be NULL) reproduces the reference's last-point value (:1535). */
int viso_get_inliers(const double* X3xM, const double* obs4xM, int m,
                     const double tr[6], const viso_param* p,
                     int32_t* inliers, int* n_inliers, double* rms);

/* ransac_minimize_reproj, src/viso.cpp:1543-1580.  samples: ransac_iter x 3
 * ascending distinct indices (what randomsample(3,m,.) :87-107 yields), or
 * NULL to draw them from viso_ransac_samples(seed, frame, ...).  best_tr is
 * in/out like the reference's: it is assigned only when a hypothesis improves the
 * support (:1564-1568), so the caller's values survive when no hypothesis finds any
 * (return 0, *n_inl = 0) and for m < 3; with a support of 1..5 it is the best
 * hypothesis' motion (return 0, :1571), otherwise the refit's (the partly iterated
 * value when the refit fails, :1572).  best_inl: up to m indices. */
int viso_ransac_minimize_reproj(const double* X3xM, const double* obs4xM, int m,
                                double best_tr[6], int32_t* best_inl, int* n_inl,
                                const viso_param* p, const int32_t* samples,
                                uint64_t seed, uint64_t frame);

/* Support sizes of n_h given motions tr_h[n_h][6] over one point set, through the RANSAC stage's counting kernel
 * (diagnostics / tests): cnt[h] = number of inliers get_inliers (src/viso.cpp:1509-1537) finds for tr_h[h]. */
int viso_support_sizes(const double* X3xM, const double* obs4xM, int m, const double* tr_h, int n_h,
                       const viso_param* p, int32_t* cnt);

/* Deterministic replacement for randomsample's per-call random_device
 * (src/viso.cpp:87-107: a uniformly distributed 3-subset of 0..m-1, ascending).
 * Triple h = the first three outputs of a splitmix64 stream keyed on
 * (seed, frame, h) through Floyd's subset sampling -- t_i = floor(draw_i * (j+1) / 2^64)
 * for j = m-3, m-2, m-1, taken, or j itself if t_i was taken already -- sorted
 * ascending: the same distribution in three draws (the reference's algorithm S
 * needs ~m/2; rounds 1-5 ran it over the same stream: other triples, same law).
 * m < 3: zeros.  out: iters x 3. */
void viso_ransac_samples(uint64_t seed, uint64_t frame, int iters, int m, int32_t* out);

/* tr2mat, src/viso.cpp:109-133. T: 4x4 row-major. Host arithmetic (six
 * sin/cos; nothing to offload). */
void viso_tr2mat(const double tr[6], double T[16]);
/* pose <- pose * inv(tr2mat(tr)), src/viso.cpp:1315-1321. */
void viso_pose_update(const double pose[16], const double tr[6], double out[16]);
/* F_from_P<double>, src/mvg.h:41-66, followed by the normalisation of
 * src/viso.cpp:1177-1180.  P1,P2: 3x4 row-major. */
void viso_F_from_P(const double P1[12], const double P2[12], double F[9]);

/* MyFeatureExtractor::computeImpl, src/viso.cpp:1004-1024: Sobel-x 3x3
 * (BORDER_REFLECT_101) then (2r+1)^2 window per keypoint; zero where
 * y<=0|y>=rows|x<=0|x>=cols.  img: rows x cols uint8.  desc: n x (2r+1)^2. */
int viso_extract_descriptors(const uint8_t* img, int rows, int cols,
                             const float* kp, int n, int radius, float* desc);

/* cv::cornerHarris(img, R, 3, 5, k, BORDER_DEFAULT) restated in OpenCV's evaluation order (scale folded into the float
 * smoothing taps, row pass then column pass with the symmetric grouping, box filter as row sums then column sums; what
 * an algorithm-level restatement cannot pin is listed in oracle/viso_oracle.c); resp: rows x cols float.
 * ($VISO_HARRIS_BAND = rows per wave of the response kernel, 1..4096: a tuning / test aid, the image does not depend on it.) */
int viso_harris_response(const uint8_t* img, int rows, int cols, double k, float* resp);
/* HarrisBinnedFeatureDetector::detectImpl, src/viso.cpp:926-975 (reference defaults:
 * n_features 1200, nbinx 24, nbiny 5).  kp: up to n_features x 2 (x,y);
 * resp_out (may be NULL): |response| per keypoint. */
int viso_detect_harris_binned(const uint8_t* img, int rows, int cols, int n_features, int nbinx, int nbiny,
                              double k, float* kp, float* resp_out, int* n_out);

/* Where a plain-family call's time goes (diagnostics; bench.py `drop_in_per_call`, viso_host_gputest).  The plain family is
 * what the patched reference loop calls once per function per frame (src/viso.cpp:1240-1313: match_desc x3,
 * collect_matches, triangulate_rectified, match_circle, ransac_minimize_reproj), so a frame's cost there is seven
 * synchronous host->device->host round trips.  With profiling on, every call brackets its phases with hipEvents on the
 * default context's stream: h2d_us = input copies, kernel_us = the kernels, d2h_us = result copies (up to the last byte
 * on the host), wait_us = host time blocked in hipStreamSynchronize / blocking copies, host_us = wall time of the call.
 * Sums over the calls since profiling was switched on.  Profiling costs a few microseconds per call: rates are quoted
 * with it off. */
#define VISO_PLAIN_MATCH_DESC 0
#define VISO_PLAIN_COLLECT_MATCHES 1
#define VISO_PLAIN_TRIANGULATE 2
#define VISO_PLAIN_MATCH_CIRCLE 3
#define VISO_PLAIN_RANSAC 4
#define VISO_PLAIN_MINIMIZE 5
#define VISO_PLAIN_GET_INLIERS 6
#define VISO_PLAIN_N 7
typedef struct viso_plain_times {
    int64_t calls;
    double host_us, h2d_us, kernel_us, d2h_us, wait_us;
} viso_plain_times;
/* What the plain family does behind one function per call (libviso_amd/csrc/plain.hip; DESIGN.md "the drop-in path"):
 *   image cache    match_desc recognises an image it has been given before -- the loop passes every (keypoints,
 *                  descriptors) set three times, under changing addresses (`d1.copyTo(d1_prev)`, src/viso.cpp:1213) -- by
 *                  comparing its bytes with a pinned host shadow (memcmp: exact), and then neither uploads nor sorts nor
 *                  packs it again.  viso_plain_cache(0) / $VISO_PLAIN_CACHE=0: every image uploaded again.
 *   frames         the stereo call of a frame (enforce_epipolar != 0) also runs what the loop asks for next: the two
 *                  temporal match_desc problems against the previous stereo call's images, collect_matches /
 *                  triangulate_rectified of its own matches, match_circle of the four lists, the gather of :1292-1305
 *                  and ransac_minimize_reproj with the parameters and stream key of the previous frame's call (key
 *                  advanced by its last step).  A later call is answered from those results ONLY if its arguments are
 *                  byte for byte what was assumed (the functions are pure: same results as the direct path, which any
 *                  other argument takes).  Guessing starts after the call sequence has been seen once and stops when a
 *                  guess goes unused.  viso_plain_speculate(0) / $VISO_PLAIN_SPECULATE=0: every call direct.
 *   waiting        a call returns when its results are in pinned host memory: the workgroups that write them there (they ride in
 *                  the launch of the chain's next kernel; the last kernel writes its own) say so in a pinned word the host
 *                  spins on (a few microseconds sooner than hipStreamSynchronize sees it; after 20 ms the stream is
 *                  synchronised instead).  $VISO_PLAIN_SIGNAL=0: always hipStreamSynchronize.
 * Both only change when the work is done, never a result (tests/test_gpu_drop_in.py runs every combination).  The
 * speculation statistics: served[0..3] = calls answered from a frame (temporal match_desc, collect_matches,
 * triangulate_rectified + match_circle, ransac_minimize_reproj), wasted[0..3] = results computed ahead and never asked for. */
int viso_plain_cache(int enable);
int viso_plain_cache_stats(int64_t* hits, int64_t* misses);
int64_t viso_plain_general_reruns(void);   /* calls repeated because their launch had left out a kernel the data then needed: an image
                                              that unexpectedly did not fit the u16 rows, or a stereo pair with a wide epipolar band
                                              after several rectified ones */
int viso_plain_speculate(int enable);
int viso_plain_speculate_stats(int64_t served_wasted[8]);
/* $VISO_PLAIN_TRACE=1: host microseconds of viso_match_desc by phase, of the temporal calls answered from a frame, and the waits of
   match_circle / ransac_minimize_reproj behind the stereo call; this prints and zeroes them (stderr). */
void viso_plain_trace_dump(void);
int viso_plain_profile(int enable);                        /* 1: zero the sums and start; 0: stop */
int viso_plain_profile_get(int fn, viso_plain_times* out); /* fn: VISO_PLAIN_* */
const char* viso_plain_profile_name(int fn);

/* ------------------------------------------- batched, device-resident family
 *
 * A frame set holds `n_frames` stereo frames resident in HBM:
 *   kp   [n_frames][2][cap][2]   float   (x,y)   image 0 = left, 1 = right
 *   desc [n_frames][2][cap][121] float            (the reference's boundary layout)
 *   n    [n_frames][2]           int32   keypoints actually present (<= cap)
 * viso_batch_* processes the pairs (t-1,t) for t = 1..n_frames-1 exactly like
 * one iteration each of sequence_odometry's loop body (src/viso.cpp:1205-1327):
 * stereo match of every frame, two temporal matches, circle join, gather,
 * RANSAC/GN.  All stages run on the context's stream without host round trips.
 */
typedef struct viso_batch viso_batch;

viso_batch* viso_batch_create(viso_ctx* ctx, int n_frames, int cap, int dlen);
/* Waits for the context's streams, frees the batch; return value as viso_ctx_destroy (VISO_OK also for a batch its context
 * has already taken along; VISO_ERR_ARG for a handle that is not, or no longer, a batch). */
int viso_batch_destroy(viso_batch* b);

/* Stream rule for everything below: a batch's kernels run asynchronously on its context's stream.  Every call
 * that writes batch inputs (upload*, set_params, detect) is ordered against that stream — the synchronous ones
 * wait for it, the *_async ones are enqueued on it — so it is safe to call them while a run is in flight.
 * Every entry point selects the context's device (hipSetDevice) first: one process may drive several GPUs. */

/* Upload host data for frames [f0, f0+nf) (layout as above, tightly packed
 * over nf frames).  Synchronous: returns when the data is on the device. */
int viso_batch_upload(viso_batch* b, int f0, int nf, const float* kp,
                      const float* desc, const int32_t* n);
/* Same, enqueued on the context's stream: returns at once.  The host buffers must stay untouched until the
 * stream has passed the copies (viso_ctx_synchronize / any result getter of a later run).  Buffers from
 * viso_host_alloc (pinned) are copied by DMA and overlap kernels of other contexts: the streaming mode of a
 * host that feeds new frames every step (sequence_odometry consumes fresh data per frame, src/viso.cpp:1205-1231). */
int viso_batch_upload_async(viso_batch* b, int f0, int nf, const float* kp,
                            const float* desc, const int32_t* n);
/* The same uploads with the descriptors as int16 (N x dlen, tightly packed over [nf][2][cap][dlen]): the lossless
 * encoding of what MyFeatureExtractor produces (3x3 Sobel of uint8: integers in [-1020, 1020], src/viso.cpp:1004-1024)
 * at half the bytes of the reference's CV_32F rows (:995,1008) — the PCIe-bound streaming mode moves half the data.
 * Same results as the f32 uploads of the same values.  All frames of a batch must come through ONE of the two
 * families (the int16 rows live in the f32 rows' device buffer): the batch remembers per frame which family filled it,
 * and viso_batch_run* returns VISO_ERR_ARG when the frames of a run disagree.  Needs dlen <= 128. */
int viso_batch_upload_i16(viso_batch* b, int f0, int nf, const float* kp,
                          const int16_t* desc16, const int32_t* n);
int viso_batch_upload_i16_async(viso_batch* b, int f0, int nf, const float* kp,
                                const int16_t* desc16, const int32_t* n);
void* viso_host_alloc(size_t bytes);
int viso_host_free(void* p);
/* Device pointers of the boundary-layout buffers, for producers that already
 * live on the GPU (a device-side extractor, torch): kp, desc, n as above. */
int viso_batch_device_ptrs(viso_batch* b, void** kp, void** desc, void** n);

int viso_batch_set_params(viso_batch* b, const viso_match_params* stereo,
                          const viso_match_params* temporal, const viso_param* p,
                          uint64_t seed, uint64_t first_frame_index);

/* Matcher stage only (BASELINE config 2): pack + 3 match_desc per frame
 * (stereo for all frames, temporal L and R for t>=1) incl. the final sort. */
int viso_batch_run_matcher(viso_batch* b);
/* Full per-frame path (BASELINE config 3): matcher + triangulation + circle
 * join + RANSAC/GN.  Asynchronous on the context's stream. */
int viso_batch_run(viso_batch* b);

/* Image-in mode: upload uint8 images [nf][2][rows][cols]
 * and keypoints; viso_batch_run_images extracts the 11x11 Sobel-x descriptor
 * windows on the device (MyFeatureExtractor, src/viso.cpp:1004-1024) straight
 * into the matcher's row format and then runs like viso_batch_run_matcher
 * (matcher_only != 0) or viso_batch_run.  Needs dlen == 121. */
int viso_batch_upload_images(viso_batch* b, int f0, int nf, const uint8_t* images, int rows, int cols,
                             const float* kp, const int32_t* n);
int viso_batch_run_images(viso_batch* b, int matcher_only);
/* viso_batch_upload_images enqueued on the stream (see viso_batch_upload_async); the image buffers must already
 * exist for this geometry (one synchronous viso_batch_upload_images call allocates them). */
int viso_batch_upload_images_async(viso_batch* b, int f0, int nf, const uint8_t* images, int rows, int cols,
                                   const float* kp, const int32_t* n);
/* HarrisBinnedFeatureDetector::detectImpl (src/viso.cpp:926-975) on every
 * uploaded image (pass kp = n = NULL to viso_batch_upload_images): fills the
 * batch's keypoints on the device, one workgroup per (image, bin), without a response image in memory (bins up to
 * 62 pixels wide with up to 32 corners each; larger ones take a response image + a selection kernel).
 * cv::cornerHarris(blockSize 3, ksize 5, k)
 * restated; the reference leaves k uninitialised (:915-919,978) — its intended
 * default is 0.04f — and the order inside a bin unspecified (:963); here:
 * (|response| desc, push order asc).  n_features/(nbinx*nbiny) corners per bin. */
int viso_batch_detect(viso_batch* b, int n_features, int nbinx, int nbiny, double k);
int viso_batch_get_keypoints(viso_batch* b, int t, int side, float* kp, int* n_out);

/* Results (host copies; they synchronise the stream).
 * which: 0 = stereo L->R of frame t, 1 = temporal left (t vs t-1), 2 = temporal right. */
int viso_batch_get_matches(viso_batch* b, int which, int t, int32_t* out_match, int* out_n);
int viso_batch_get_circle(viso_batch* b, int t, int32_t* circ, int32_t* pcl, int* out_n);
/* tr[6], ok (1/0, 0 also when <3 circle matches, src/viso.cpp:1283), inliers. */
int viso_batch_get_pose(viso_batch* b, int t, double tr[6], int* ok,
                        int32_t* inliers, int* n_inl);
/* All frames at once: tr [n_frames][6], ok [n_frames], n_inl [n_frames]
 * (entry 0 is zero/0: the first frame has no predecessor, :1256-1260).  Waits for the batch's streams, then reads a
 * pinned host mirror that the last kernel of every viso_batch_run / viso_batch_run_images fills: no device copy. */
int viso_batch_get_poses(viso_batch* b, double* tr, int32_t* ok, int32_t* n_inl);
/* Per-hypothesis state of the last run's RANSAC stage (diagnostics / tests): tr_h [n_frames][ransac_iter][6],
 * ok_h, cnt_h [n_frames][ransac_iter] (support sizes; frame 0 unused), *n_undecided = hypotheses that needed the
 * wave-per-hypothesis kernel.  Any pointer may be NULL.  ransac_iter is the one given to viso_batch_set_params;
 * viso_batch_get_hypotheses2 takes the capacity of the caller's arrays (in hypotheses per frame): the arrays are
 * [n_frames][iters_capacity] (x 6 for tr_h) and every frame's row is written at THAT stride (entries beyond ransac_iter
 * are left alone); VISO_ERR_ARG when iters_capacity < ransac_iter. */
int viso_batch_get_hypotheses(viso_batch* b, double* tr_h, int32_t* ok_h, int32_t* cnt_h, int32_t* n_undecided);
int viso_batch_get_hypotheses2(viso_batch* b, int iters_capacity, double* tr_h, int32_t* ok_h, int32_t* cnt_h,
                               int32_t* n_undecided);
/* Work counters of the last run, for the algorithmic-bytes model of
 * per (which,t) the number of scored (query,candidate) pairs C
 * and matches emitted M_out.  scored/m_out: [3][n_frames] int64. */
int viso_batch_get_counters(viso_batch* b, int64_t* scored, int64_t* m_out);
/* flags [n_frames][2]: 1 where the last run found descriptor values of that image that the packed u16 rows cannot
 * hold (not integers in [-32768, 32767], or dlen > 128).  Only the match_desc calls that read such an image take
 * the general kernel (float differences summed in double, the arithmetic of cv::norm at src/viso.cpp:702); all
 * other calls of the batch stay on the u16 kernels.  Same results either way. */
int viso_batch_get_general_path_flags(viso_batch* b, int32_t* flags);
/* Number of queries of the last run that took match_overflow_kernel (exact K-cap selection / largest-key tie rule
 * / candidate lists beyond the tile kernels' LDS slots): a few for sparse features, a sizeable share where keypoints
 * cluster densely.  Same results either way; this is the data-dependent cost to watch. */
int viso_batch_get_overflow_count(viso_batch* b, int32_t* n);
/* Diagnostics: the shift of the 8-bit planes the batch's last run used (viso_ctx_set_row8_shift). */
int viso_batch_get_row8_shift(viso_batch* b, int* shift);
/* Duration of the kernel that takes the temporal calls (viso_ctx_matcher_kernel_name), measured with hipEvents
 * on the context's stream: average in ms over the runs since the last viso_batch_kernel_ms call. */
int viso_batch_kernel_timing(viso_batch* b, int enable);
int viso_batch_kernel_ms(viso_batch* b, double* matcher_ms_avg, int* n_launches);
/* Time stamps of a run (hipEvents on the batch's streams), for hosts that want to know where a chunk's time went
 * (the KITTI runner's per-rank report): viso_batch_stamp(b, 0) before the run's uploads, viso_batch_stamp(b, 1) after
 * them; viso_batch_run* stamps the end of the run itself.  viso_batch_stamp_ms waits for the run and returns
 * ms[0] = the uploads, ms[1] = everything the run launched behind them. */
int viso_batch_stamp(viso_batch* b, int which);
int viso_batch_stamp_ms(viso_batch* b, double ms[2]);

/* ------------------------------------------------ sub-pixel stereo refinement (opt-in; NOT in the reference)
 *
 * Every stereo correspondence of the reference is an integer pixel pair (Harris keypoints are Point2f(int,int),
 * src/viso.cpp:967), and collect_matches / triangulate_rectified turn that integer disparity straight into depth
 * (:501-514, :1137-1162).  With this on, the right-image point of every stereo match is refined to sub-pixel precision
 * by a parabola through the descriptor-window SADs at the match and its two neighbours.  Definition, for a stereo row
 * (i1, i2, dist) of frame t as viso_batch_get_matches(b, 0, t, ...) returns it:
 *   p = (cvRound(kp1[i1].x), cvRound(kp1[i1].y)), q = (cvRound(kp2[i2].x), cvRound(kp2[i2].y))   (rounding half to even,
 *       as MyFeatureExtractor, src/viso.cpp:1013);
 *   W_L(p) = the left descriptor window, W_R(x, y) = the right image's window at (x, y): exactly viso_extract_descriptors
 *       (Sobel-x with BORDER_REFLECT_101, 11x11, each pixel zeroed where y<=0 | y>=rows | x<=0 | x>=cols) at that point;
 *   Sx(d) = SAD(W_L(p), W_R(q.x+d, q.y)), Sy(d) = SAD(W_L(p), W_R(q.x, q.y+d)), d in {-1, 0, +1}: int32, exact
 *       (Sx(0) = Sy(0) = the row's dist);
 *   off(S-, S0, S+) = (double)(S- - S+) / (2.0 * (double)(S- + S+ - 2*S0)) when S0 <= S-, S0 <= S+ and S- + S+ - 2*S0 > 0,
 *       else 0 (so |off| <= 1/2); IEEE double, no contraction;
 *   uR' = (float)((double)q.x + off(Sx)); vR' = (float)((double)q.y + off(Sy)) in mode 2, (float)q.y in mode 1.
 * The left point is not changed.  Modes: 0 = off (the default), 1 = horizontal only (disparity), 2 = horizontal and vertical.
 *
 * In a batch (image-in runs only), subpixel_refine_kernel refines every frame's final stereo list once per run, and the circle
 * join takes the right-image observation of x_c (rows 2-3) from frame t's refined point of the joined stereo row and
 * triangulates Xp_c with frame t-1's refined uR.  Match lists, the circle join's rows and the RANSAC stream key (seed,
 * first_frame + t) are those of mode 0; poses are not comparable with the reference's.  Mode 0 runs exactly the kernels
 * and arithmetic of the reference path. */

/* mode 0, 1 or 2 for the batch's next runs.  viso_batch_run_images (matcher_only included) then refines; viso_batch_run /
 * viso_batch_run_matcher (descriptor-in frames: no images to refine on) return VISO_ERR_ARG while mode != 0, and the batch
 * stays usable. */
int viso_batch_set_subpixel(viso_batch* b, int mode);
/* The refined points of frame t's stereo rows from the last run: uv [n][2] float (uR', vR'), in the order of
 * viso_batch_get_matches(b, 0, t, ...); *out_n = n.  VISO_ERR_ARG when the last run refined nothing (mode 0, or a
 * descriptor-in run).  Synchronises like the other getters. */
int viso_batch_get_subpixel(viso_batch* b, int t, float* uv, int* out_n);
/* The same refinement for host pointers on the default context (single calls, tests): imgL / imgR rows x cols uint8,
 * kp1 n1 x 2, kp2 n2 x 2 float (x,y), match n x 3 int32 (i1, i2, dist) with 0 <= i1 < n1, 0 <= i2 < n2; mode 1 or 2.
 * out_uv: n x 2 float (uR', vR') per row of match. */
int viso_refine_stereo_subpixel(const uint8_t* imgL, const uint8_t* imgR, int rows, int cols, const float* kp1, int n1,
                                const float* kp2, int n2, const int32_t* match, int n, int mode, float* out_uv);

/* ------------------------------------------------ rectification of raw camera images (opt-in; NOT in the reference)
 *
 * Every stage assumes undistorted, rectified pairs (triangulate_rectified, src/viso.cpp:1137-1162; the Sampson gate around
 * F_from_P(P1, P2)); KITTI odometry ships them, other rigs and KITTI raw's unrectified drives do not.  With this on, the batch's
 * image uploads take RAW images and a HIP kernel (rectify_remap_kernel) undistorts and rectifies them into the image buffer the
 * detector, the extractor, the matchers and the sub-pixel refinement read; none of those changes.
 *
 * Map of one camera: mapx, mapy [out_rows][out_cols] float, the raw-image position output pixel (x, y) samples (pixel centres at
 * integer coordinates, the convention of the extractor and Harris).  viso_rectify_map builds it with the plumb-bob model in the
 * form of OpenCV's initUndistortRectifyMap, in double: K 3x3 (K[0][1] must be 0), D = (k1, k2, p1, p2, k3), R 3x3 the
 * rectifying rotation, P 3x4 of which only the left 3x3 P33 is used:
 *   iR = inverse(P33 R); (x', y', w) = iR (x, y, 1); x' /= w; y' /= w; r2 = x'^2 + y'^2; kr = 1 + k1 r2 + k2 r2^2 + k3 r2^3;
 *   xd = x' kr + 2 p1 x' y' + p2 (r2 + 2 x'^2); yd = y' kr + p1 (r2 + 2 y'^2) + 2 p2 x' y';
 *   mapx = (float)(K00 xd + K02); mapy = (float)(K11 yd + K12).
 * (Held to a tolerance, not to bit equality; K = P33, D = 0, R = I gives mapx = x, mapy = y exactly.)
 * Quantisation (host, when a map is installed): X = lrintf(mapx * 32) (ties to even), ix = X >> 5 (floor), fx = X & 31, the
 * same for y; an entry that is not finite or has |map| >= 32768 is OUTSIDE: its output is the border value and it loads nothing.
 * Remap (device, integer, exact), with tap(a, b) = raw[iy+b][ix+a] when 0 <= ix+a < raw_cols and 0 <= iy+b < raw_rows, else border:
 *   out = ((32-fx)(32-fy) tap(0,0) + fx(32-fy) tap(1,0) + (32-fx) fy tap(0,1) + fx fy tap(1,1) + 512) >> 10   (<= 255).
 * Bilinear at 1/32 pixel like OpenCV's INTER_LINEAR, whose 15-bit weight tables can differ from this by one LSB: the result is
 * not claimed equal to OpenCV's remap.
 *
 * In a batch one launch rectifies all frames of an upload: each workgroup keeps its output tile's map entries in registers and
 * loops over a chunk of 32 of the upload's frames, so a caller that uploads one frame at a time re-reads the maps (8 B per
 * output pixel and camera) for every frame; upload several frames per call where possible.  Outside entries and taps beyond the raw image are
 * resolved on the host before any address is formed: no map makes the kernel read out of bounds. */

/* The map of one camera (host only, no device; see above).  K 9, D 5, R 9, P 12 doubles, row-major; mapx, mapy
 * out_rows x out_cols.  VISO_ERR_ARG: sizes <= 0, a null pointer, K[0][1] != 0, or P33 R singular. */
int viso_rectify_map(const double K[9], const double D[5], const double R[9], const double P[12], int out_rows, int out_cols,
                     float* mapx, float* mapy);
/* Install (all four maps non-NULL, each out_rows x out_cols) or remove (all four NULL) rectification for the batch's NEXT image
 * uploads; synchronises like the other synchronous setters.  While it is on:
 *   - viso_batch_upload_images(_async) take raw images [nf][2][raw_rows][raw_cols]; a rows / cols other than the raw geometry
 *     returns VISO_ERR_ARG and the batch stays usable;
 *   - an upload copies into a raw staging buffer of the batch and enqueues the remap on the context's stream (the stream rule
 *     and the async host-buffer rule of the uploads hold unchanged);
 *   - keypoints passed with an upload are in rectified coordinates; viso_batch_detect and the runs see out_rows x out_cols images.
 * Descriptor-in uploads and runs are unaffected; with rectification never installed every call launches what it launched
 * before.  VISO_ERR_ARG: sizes <= 0, border outside 0..255, some but not all maps NULL. */
int viso_batch_set_rectify(viso_batch* b, int raw_rows, int raw_cols, int out_rows, int out_cols, const float* mapxL,
                           const float* mapyL, const float* mapxR, const float* mapyR, int border);
/* The batch's device image of frame t, side (0 left, 1 right): img_rows x img_cols bytes, rectified when rectification was on at
 * its upload.  Synchronises like the other getters. */
int viso_batch_get_image(viso_batch* b, int t, int side, uint8_t* out);
/* The geometry of those images (img_rows x img_cols, what viso_batch_get_image copies): the last image upload's, or the
 * output geometry of viso_batch_set_rectify; 0 x 0 before either. */
int viso_batch_get_image_geometry(viso_batch* b, int* rows, int* cols);
/* Host pointers, default context, the batch's kernel: n raw images raw_rows x raw_cols of ONE camera -> n rectified images
 * out_rows x out_cols (out).  Same argument rules as viso_batch_set_rectify. */
int viso_rectify_images(const uint8_t* raw, int n, int raw_rows, int raw_cols, const float* mapx, const float* mapy, int out_rows,
                        int out_cols, int border, uint8_t* out);

/* ------------------------------------------------ motion covariance (opt-in; NOT in the reference)
 *
 * For one frame: L = the final inlier list (ascending point indices, what viso_batch_get_pose returns), n = |L|; tr the frame's
 * final motion; (f, cu, cv, b) from viso_param; j = 0..n-1 the position in L, k = L[j] the point; X = (X, Y, Z) the
 * previous-frame point k, Xc = R(tr) X + t (Xc, Yc, Zc).
 *   J_j   4x6  d pred_k / d tr at tr: compute_J (src/viso.cpp:1401-1497) without the weight;
 *   r_j   4    obs[:,k] - pred_k (unweighted);
 *   w_j        1 / (|obs[0][j] - cu| / |cu| + 0.05): the estimator's weight of the j-th entry -- column j, not k (Q6);
 *   T_k   3x3  dX / d(uL, vL, uR) of the previous frame's triangulation (src/viso.cpp:1137-1162), d = f b / Z, columns
 *              (b/d - X/d, -Y/d, -Z/d), (0, b/d, 0), (X/d, Y/d, Z/d)  (vR is not used by triangulation);
 *   Jx_j  4x3  d pred / d X = Pc R, Pc rows uL (f/Zc, 0, -f Xc/Zc^2), vL (0, f/Zc, -f Yc/Zc^2),
 *              uR (f/Zc, 0, -f (Xc-b)/Zc^2), vR = the vL row;
 *   M_j = Jx_j T_k  4x3.
 * Under iid pixel noise sigma^2 on every keypoint coordinate of both frames:
 *   A = sum w_j^2 J_j'J_j,  B = sum w_j^4 J_j' (I4 + M_j M_j') J_j,  cov = sigma^2 A^-1 B A^-1  (the weighted estimator's sandwich;
 *   parameter order of tr: rx, ry, rz in rad, tx, ty, tz in units of base);
 *   g = sum w_j^2 J_j' r_j,  delta = A^-1 g (the step to the weighted least-squares optimum the reported tr may stop short of:
 *   the reference's convergence test fabs(p > thresh), :1610, leaves a large negative step unapplied),
 *   gap = g' B^-1 g / sigma^2 (= delta' cov^-1 delta; 0 when sigma^2 = 0).  tr itself is never changed.
 * sigma^2: mode 1 estimates it, sigma2 = sum |r_j|^2 / (sum (4 + |M_j|_F^2) - 6); mode 2 takes sigma_px^2 from the caller
 * (finite and > 0, else VISO_ERR_ARG); mode 0 is off (the default: every run launches what it launched before).
 * status 1 valid; 0 no pose (frame 0, or ok == 0); -1 n < 6; -2 A or B not positive definite (a Cholesky pivot that is not
 * > 1e-12 x the original diagonal entry).  When status != 1, cov, delta, sigma2 and gap are zeros.
 * One HIP kernel (motion_cov_kernel) serves every path; its summation order depends on n only (fixed DPP and LDS trees, no
 * atomics), so the batch at any chunking and the direct call give byte-identical records for the same inputs. */
typedef struct viso_motion_cov {
    double cov[36];     /* 6 x 6 row-major, symmetric */
    double delta[6];
    double sigma2;
    double gap;
    int32_t status;
    int32_t n;          /* |L| */
} viso_motion_cov;

/* mode 0 (off), 1 (estimated sigma) or 2 (sigma = sigma_px) for the batch's next runs: viso_batch_run and viso_batch_run_images
 * (not matcher_only) then launch motion_cov_kernel on the RANSAC stream behind the refit.  VISO_ERR_ARG: another mode, or mode 2
 * with a sigma_px that is not finite and > 0. */
int viso_batch_set_covariance(viso_batch* b, int mode, double sigma_px);
/* The record of frame t / of all n_frames frames (frame 0: status 0) from the last run.  VISO_ERR_ARG when the last run computed
 * none (mode 0, or matcher_only); the batch stays usable.  Synchronise like the other getters. */
int viso_batch_get_covariance(viso_batch* b, int t, viso_motion_cov* out);
int viso_batch_get_covariances(viso_batch* b, viso_motion_cov* out /* [n_frames] */);
/* Frame t's solver inputs from the last run: X3xcap [3][cap] the previous-frame points, obs4xcap [4][cap] (uL, vL, uR, vR), rows of
 * cap doubles of which the first *m columns are set (either pointer may be NULL).  Synchronises like the other getters. */
int viso_batch_get_points(viso_batch* b, int t, double* X3xcap, double* obs4xcap, int* m);
/* Host pointers, default context, the batch's kernel: X 3 x m, obs 4 x m (row-major), tr 6, inl n_inl indices in [0, m) with
 * n_inl <= m; mode 1 or 2.  The pose counts as solved (ok = 1). */
int viso_pose_covariance(const double* X, const double* obs, int m, const double tr[6], const int32_t* inl, int n_inl,
                         const viso_param* param, int mode, double sigma_px, viso_motion_cov* out);
/* Host only (no device).  Propagates the records along hostmath.chain_poses' list: entry 0 is the identity (zero covariance);
 * every frame t with ok[t] != 0 appends P_k = P_{k-1} inv(T_k), T_k = tr2mat(tr[t]).  With the right perturbation P = P^ Exp(xi),
 * xi = (phi, rho), rotation first:
 *   S_k = Ad(T_k) S_{k-1} Ad(T_k)' + G_k cov_t G_k',  Ad(T) = [[R, 0], [t^ R, R]],  G_k = d Log(T_k inv(T(tr))) / d tr at tr[t].
 * An entry is valid until the first chained frame whose status != 1 and invalid (zeros) from there on.  tr n x 6, ok n, cov n;
 * pose_cov36 and valid hold n + 1 entries; *n_out = the number of entries written. */
int viso_chain_covariances(const double* tr, const int32_t* ok, const viso_motion_cov* cov, int n, double* pose_cov36,
                           int32_t* valid, int* n_out);

/* ------------------------------------------------ motion refinement (opt-in; NOT in the reference)
 *
 * A two-frame stereo bundle adjustment: the maximum-likelihood motion and structure under iid pixel noise in both frames.  For one
 * frame with a solved pose (ok = 1): L = the final inlier list, tr the final motion, (f, cu, cv, b) from viso_param.
 *   L'  the entries k of L whose input X[:,k] is finite with Z > 0, in L's order; n = |L'| (fixed: no inlier is re-selected).
 *   Unknowns tr (6, tr2mat's convention) and X_k (3) for k in L', starting at the frame's tr and the input X.
 *   z0_k = (f X/Z + cu, f Y/Z + cv, f (X-b)/Z + cu) of the input X_k: the previous frame's observations, triangulate_rectified
 *          inverted (sub-pixel disparities are honoured; vR of the previous frame is not used, as in the covariance);
 *   r0_k = z0_k - pi0(X_k) (pi0 the same three expressions), r1_k = obs[:,k] - pred(tr, X_k) (4 rows, compute_J's prediction);
 *   C = sum |r0|^2 + sum |r1|^2, unweighted (the reference's w_j and its Q6 column play no part).
 *   J_k 4x6 compute_J without the weight; Jx_k = Pc R 4x3 (the covariance's); P0_k 3x3 rows (f/Z, 0, -fX/Z^2),
 *   (0, f/Z, -fY/Z^2), (f/Z, 0, -f(X-b)/Z^2).
 *   Hcc = sum J'J, Hcp_k = J_k'Jx_k, Hpp_k = Jx_k'Jx_k + P0_k'P0_k, gc = sum J'r1, gp_k = Jx_k'r1_k + P0_k'r0_k;
 *   S = Hcc - sum Hcp_k Hpp_k^-1 Hcp_k', s = gc - sum Hcp_k Hpp_k^-1 gp_k; S dtr = s, dX_k = Hpp_k^-1 (gp_k - Hcp_k' dtr).
 * Levenberg-Marquardt: the diagonals of Hcc and of every Hpp_k are multiplied by (1 + lambda), lambda_0 = 1e-4.  A candidate with a
 * strictly lower C is accepted (lambda = max(lambda / 10, 1e-12)), otherwise lambda *= 10.  Stop after 8 consecutive rejections,
 * after 20 accepted steps, after an accepted step with C_old - C_new <= 1e-12 C_old, or when C == 0.
 * At the final state, undamped: cov = sigma^2 S^-1 (the motion's marginal covariance), gap = s'S^-1 s / sigma^2 (~ 0 at
 * convergence; 0 when sigma^2 = 0).  sigma^2: mode 1 C / (4n - 6), mode 2 sigma_px^2 (finite and > 0, else VISO_ERR_ARG);
 * mode 0 is off (the default: every run launches what it launched before).
 * status 1 valid; 0 no pose (frame 0, or ok == 0); -1 n < 6; -2 a Cholesky pivot of S, of an Hpp_k (damped while iterating) or of
 * a point's I - M M' (M = Jx~ l^-T; positive definite in exact arithmetic) is not > 1e-12 x its diagonal entry; -3 a non-finite value appeared (C at the start, the sums of S and s, the final record; a
 * candidate whose C is not finite is rejected).  When status != 1, tr is the input tr, n is |L'| and every other field is zero:
 * a consumer can always chain rec.tr where ok.  The batch's tr, ok, inliers and covariance records are never changed.
 * One HIP kernel (motion_refine_kernel) serves every path; its summation order depends on n only (fixed DPP and LDS trees, no
 * atomics), so the batch at any chunking and the direct call give byte-identical records for the same inputs. */
typedef struct viso_motion_refine {
    double tr[6];
    double cov[36];     /* 6 x 6 row-major, symmetric */
    double sigma2;
    double cost0;       /* C at the start */
    double cost;        /* C at the end */
    double gap;
    int32_t iters;      /* accepted steps */
    int32_t status;
    int32_t n;          /* |L'| */
    int32_t _pad;
} viso_motion_refine;

/* mode 0 (off), 1 (estimated sigma) or 2 (sigma = sigma_px) for the batch's next runs: viso_batch_run and viso_batch_run_images
 * (not matcher_only) then launch motion_refine_kernel on the RANSAC stream behind the refit (and behind the covariance when on).
 * VISO_ERR_ARG: another mode, or mode 2 with a sigma_px that is not finite and > 0. */
int viso_batch_set_refine(viso_batch* b, int mode, double sigma_px);
/* The record of frame t / of all n_frames frames (frame 0: status 0) from the last run.  VISO_ERR_ARG when the last run computed
 * none (mode 0, or matcher_only); the batch stays usable.  Synchronise like the other getters. */
int viso_batch_get_refine(viso_batch* b, int t, viso_motion_refine* out);
int viso_batch_get_refines(viso_batch* b, viso_motion_refine* out /* [n_frames] */);
/* Frame t's refined points from the last run, in L' order: idx [cap] the point indices k, X3xcap [3][cap] rows of cap doubles, the
 * first *n columns set (*n = 0 when the record's status != 1; either pointer may be NULL).  VISO_ERR_ARG as viso_batch_get_refine. */
int viso_batch_get_refined_points(viso_batch* b, int t, int32_t* idx, double* X3xcap, int* n);
/* Host pointers, default context, the batch's kernel: X 3 x m, obs 4 x m (row-major), tr 6, inl n_inl indices in [0, m) with
 * n_inl <= m; mode 1 or 2.  The pose counts as solved (ok = 1).  Xout (may be NULL): 3 rows of n_inl doubles, the first out->n
 * columns the refined points in L' order when status is 1. */
int viso_pose_refine(const double* X, const double* obs, int m, const double tr[6], const int32_t* inl, int n_inl,
                     const viso_param* param, int mode, double sigma_px, viso_motion_refine* out, double* Xout);

/* ------------------------------------------------ window refinement (opt-in; NOT in the reference)
 *
 * A causal (fixed-lag) sliding-window stereo bundle adjustment over feature tracks.  Per frame j >= 1 of the batch:
 * circ[j] rows (cur-left, cur-right, prev-left, prev-right), x_c[j] (4 x m) and Xp_c[j] (3 x m) (column i belongs to row i), ok_j,
 * tr_j, the final inlier list L_j and L'_j (the motion refinement's set: the entries of L_j whose Xp_c column is finite with Z > 0,
 * in L_j's order).
 *   Window: K in 2..5.  A frame j >= 1 is a break when ok_j = 0 or |L'_j| < 6.  For frame t: status 0 when t = 0 or ok_t = 0, -1
 *   when |L'_t| < 6 (in these cases the window is not formed); otherwise the anchor is a = max(t - K + 1, 0, the largest break
 *   j < t), the window is frames a..t, len = t - a + 1 >= 2.  It never reaches before the batch's frame 0: a chunked sequence gives
 *   the unchunked records when each chunk begins K - 1 frames early (the halo).
 *   Links: a row r of L'_j, a + 1 < j <= t, with prev-left p links to the row r' of L'_{j-1} with cur-left p when r is the only row
 *   of L'_j with prev-left p and r' the only row of L'_{j-1} with cur-left p (no forks).  Frame a's own rows are never used.
 *   Tracks: the maximal chains r_{s+1} in L'_{s+1}, ..., r_e in L'_e of linked rows, a <= s < e <= t; every row of every L'_j,
 *   a < j <= t, is in exactly one.  Order: s ascending, then L'_{s+1}'s order.  Observations: frame s gives z0 = pi0 of
 *   Xp_c[s+1][:, r_{s+1}] (the motion refinement's three rows), every frame j in (s, e] gives x_c[j][:, r_j] (four rows).
 *   Unknowns: tr_{a+1..t} (tr2mat's convention, starting at the batch's tr) and one point X per track in frame a's coordinates,
 *   starting at Xp_c[s+1][:, r_{s+1}] mapped by the inverse of the starting T_s; T_j = M(tr_j) ... M(tr_{a+1}), T_a = I.
 *   Predictions: pi0(T_s X) for frame s, compute_J's prediction of T_j X for j > s.  C = the sum of the squared unweighted residuals.
 *   n_points = the number of tracks, n_rows = sum over the tracks of 3 + 4 (e - s).
 * Levenberg-Marquardt as the motion refinement's (lambda_0 = 1e-4, x (1 + lambda) on the diagonals of the 6 (len - 1) square camera
 * block and of every point's Hpp, the same accept, reject and stop rules); the camera block is solved through its Schur complement
 * S, s.  Per-point guards (status -2 when a pivot is not > 1e-12 x its diagonal entry): the Cholesky factor l of the damped Hpp;
 * for a track with s = a, I - M'M with M = Jx~ l^-T over its camera-dependent rows (the nonzero spectrum of the motion
 * refinement's I - M M'; a track with s > a has no camera-free rows, its I - M M' is only semi-definite at lambda = 0 and is not
 * tested).  At the final state, undamped: cov = sigma^2 x the tr_t block of S^-1, gap = s'S^-1 s / sigma^2 over the whole camera
 * block.  sigma^2: mode 1 C / (n_rows - 3 n_points - 6 (len - 1)) (status -1 when that denominator is <= 0, in either mode), mode 2
 * sigma_px^2.  status 1 valid, 0, -1, -2 (a pivot of S or of a point's block), -3 (non-finite: C at the start, the sums of S and s,
 * the final record).  When status != 1: tr is tr_t, tr_win the input tr_{a+1..t}, len / n_points / n_rows are set (all three 0
 * when the window is not formed), every other field is zero.
 * Identity: at len = 2 the definition is the motion refinement's, so a K = 2 record's tr, cov, sigma2, cost0, cost, gap, iters and
 * status agree with viso_motion_refine's to the bounds of two summation orders.  The batch's tr, ok, inliers, covariance and
 * motion refinement records are never changed.  Two HIP kernels serve every path (window_links_kernel, window_refine_kernel); the
 * summation order depends on the window's inputs only (fixed DPP and LDS trees, no float atomics), so the batch at any chunking
 * with a K - 1 halo and the direct call give byte-identical records. */
typedef struct viso_window_record {
    double tr[6];        /* the refined tr_t */
    double cov[36];      /* 6 x 6 row-major, symmetric */
    double tr_win[4][6]; /* the refined tr_{a+1..t}, oldest first, zeros beyond len - 1 */
    double sigma2;
    double cost0;
    double cost;
    double gap;
    int32_t iters;       /* accepted steps */
    int32_t status;
    int32_t len;
    int32_t n_points;
    int32_t n_rows;
    int32_t _pad;
} viso_window_record;

/* K = 0 (off, the default: every run launches what it launched before) or K in 2..5 with mode 1 (estimated sigma) or 2 (sigma =
 * sigma_px, finite and > 0) for the batch's next runs (viso_batch_run, viso_batch_run_images unless matcher_only): they launch the
 * window kernels on the RANSAC stream behind the refit (and the covariance and motion refinement when on).  The working buffers
 * are allocated (zeroed) on the first request with K > 0, and again when a larger K is asked for.  VISO_ERR_ARG: another K, a bad
 * mode or sigma_px, a dead handle; the batch stays usable. */
int viso_batch_set_window_refine(viso_batch* b, int K, int mode, double sigma_px);
/* The record of frame t / of all n_frames frames from the last run (frame 0: status 0).  VISO_ERR_ARG when the last run computed
 * none (K = 0, or matcher_only); the batch stays usable.  Synchronise like the other getters. */
int viso_batch_get_window_refine(viso_batch* b, int t, viso_window_record* out);
int viso_batch_get_window_refines(viso_batch* b, viso_window_record* out /* [n_frames] */);
/* The direct call (host pointers, default context, the batch's kernels): the record of the last frame of a window of len frames
 * (2..5) with K = len.  Frame 0's rows are never used, so only frames 1..len-1 are passed, concatenated: m[len-1] rows each; X the
 * 3 x m_j blocks (row-major, block after block), obs the 4 x m_j blocks, left (cur-left, prev-left) per row (keypoint indices in
 * [0, 2^20)), tr [len-1][6], inl the lists (n_inl[len-1] indices in [0, m_j) each).  Every frame counts as ok = 1; the break rule
 * still applies.  mode 1 or 2 as viso_batch_set_window_refine. */
int viso_window_refine(int len, const int* m, const double* X, const double* obs, const int32_t* left, const double* tr,
                       const int32_t* inl, const int* n_inl, const viso_param* param, int mode, double sigma_px,
                       viso_window_record* out);

/* ------------------------------------------------ dense stereo disparity (opt-in; NOT in the reference)
 *
 * A per-pixel disparity map of a rectified pair, in the form of OpenCV's StereoBM (XSOBEL prefilter, SAD block, texture
 * threshold, uniqueness ratio, 1/16-px V-fit) with an order-free variant of its left-right check.  Parity with OpenCV is not
 * pinned; this definition is the contract, and the device output is bit-identical to it (exact integers throughout).
 * Inputs: rectified uint8 L, R [rows][cols]; parameters D = num_disp, B = block, c = prefilter_cap, T = texture_threshold,
 * u = uniqueness, m = lr_max_diff.  Valid: D in 16, 32, ..., 256; B odd in 5..21; c in 1..63; T >= 0; u in 0..100; m = -1 or
 * 0..D.  Any other value gives VISO_ERR_ARG.
 *   1. Prefilter: G = SobelX(I) exactly as the extractor computes it (3x3, BORDER_REFLECT_101 on both axes, an integer in
 *      [-1020, 1020]); P = clamp(G, -c, c) + c, in [0, 2c].
 *   2. r = B / 2.  A pixel (x, y) is inside when r <= y < rows - r and r <= x < cols - r; every other pixel is invalid (images
 *      smaller than the block are all invalid; not an error).  Candidates of an inside pixel: d in [0, dmax(x)],
 *      dmax(x) = min(D - 1, x - r).
 *   3. Cost C(x, y, d) = sum_{|i|,|j| <= r} |P_L(x+i, y+j) - P_R(x+i-d, y+j)|, exact; at most 2c B^2 <= 55 566 (fits 16 bits).
 *   4. d* = the smallest d that minimises C over the candidates; S = C(d*).
 *   5. Texture: invalid if sum over the window of |P_L - c| < T.
 *   6. Uniqueness (u > 0 only): thr = S + (S u) / 100 (integer division); invalid if some candidate d with |d - d*| > 1 has
 *      C(d) <= thr.
 *   7. Sub-pixel: when 0 < d* < dmax(x), p = C(d*+1), n = C(d*-1), k = p + n - 2S + |p - n|, off = k ? ((n - p) 256) / k : 0
 *      (C division, truncating toward zero; |off| <= 128); else off = 0.  disp16 = (256 d* + off + 8) >> 4, in 1/16 px.
 *      (StereoBM writes p - n: its cost index runs the other way.)
 *   8. Left-right check (m >= 0 only): for a right pixel xr >= r, dR(xr, y) = the smallest d in [0, D-1] that minimises
 *      C(xr + d, y, d) over the d with xr + d < cols - r, taken over every inside left pixel, valid or not (so the check does not
 *      depend on an order); invalid if |dR(x - d*, y) - d*| > m.
 *   9. Output int16 [rows][cols]: disp16 for valid pixels, VISO_DISP_INVALID (-16, StereoBM's value for a minimum disparity of 0)
 *      otherwise.
 * Out of scope: a negative minimum disparity.  SGM and the speckle filter are stages of their own (the next two sections).
 * One HIP kernel (stereo_disparity_kernel, one launch per batch) computes every frame of a call: one workgroup per row and
 * frame, the cost volume never written to memory.  This build handles cols <= 2048 (VISO_ERR_UNSUPPORTED beyond). */
#define VISO_DISP_INVALID (-16)
typedef struct viso_disparity_params {
    int32_t num_disp;           /* D */
    int32_t block;              /* B */
    int32_t prefilter_cap;      /* c */
    int32_t texture_threshold;  /* T */
    int32_t uniqueness;         /* u, percent */
    int32_t lr_max_diff;        /* m; -1 turns the left-right check off */
} viso_disparity_params;

/* D = 128, B = 11, c = 31, T = 10, u = 15, m = 1.  Host only. */
void viso_disparity_params_default(viso_disparity_params* p);
/* Host pointers, default context: the map of one pair (out rows x cols int16).  The arguments are checked before any device is
 * touched: VISO_ERR_ARG for null pointers, sizes <= 0 or invalid parameters; VISO_ERR_UNSUPPORTED for cols > 2048. */
int viso_stereo_disparity(const uint8_t* left, const uint8_t* right, int rows, int cols, const viso_disparity_params* params,
                          int16_t* out);
/* Turn dense disparity on with a copy of *params (off with NULL, the default) for the batch's next image-in runs:
 * viso_batch_run_images (also with matcher_only) then launches the kernel on the context's stream after the rest of the run
 * has been issued (the solver does not wait behind it; it is outside the run's time stamps), over the resident images (the rectified ones when rectification is on); poses, matches and every other output are unchanged, and with it
 * off nothing new is launched.  viso_batch_run and viso_batch_run_matcher (descriptor-in: no images) return VISO_ERR_ARG while it
 * is on, and the batch stays usable.  The output [n_frames][rows][cols] int16 is allocated when first needed and again whenever
 * the image geometry changes.  VISO_ERR_ARG: invalid parameters, a dead handle. */
int viso_batch_set_disparity(viso_batch* b, const viso_disparity_params* params);
/* Only the disparity of every frame, over images uploaded without keypoints (viso_batch_upload_images with kp = n = NULL).
 * VISO_ERR_ARG when disparity is off or no images are uploaded; VISO_ERR_UNSUPPORTED for images wider than 2048. */
int viso_batch_run_disparity(viso_batch* b);
/* The map of frame t / of all n_frames frames (rows x cols int16 each, viso_batch_get_image_geometry) from the last run that
 * computed one.  VISO_ERR_ARG when disparity is off or no run has computed it yet.  Synchronise like the other getters. */
int viso_batch_get_disparity(viso_batch* b, int t, int16_t* out);
int viso_batch_get_disparities(viso_batch* b, int16_t* out /* [n_frames][rows][cols] */);

/* ------------------------------------------------ semi-global matching (opt-in; NOT in the reference)
 *
 * A second method for the same dense maps: census costs smoothed along 4 or 8 image paths (Hirschmueller's SGM), then the
 * selection of the block matcher above on the summed costs.  Parity with any other SGM implementation is not pinned; this
 * definition is the contract, and the device output is bit-identical to it (exact integers throughout).
 * Inputs: rectified uint8 L, R [rows][cols]; parameters D = num_disp, P1 = p1, P2 = p2, paths, u = uniqueness, m = lr_max_diff.
 * Valid: D in 16, 32, ..., 256; 1 <= P1 <= P2 <= 192; paths 4 or 8; u in 0..100; m = -1 or 0..D.  Any other value gives
 * VISO_ERR_ARG.
 *   1. Census: a window 9 wide x 7 tall, rows and columns outside the image replicated (coordinates clamped).  Bit (i, j) of
 *      cen(x, y), |i| <= 4, |j| <= 3, (i, j) != (0, 0), is 1 when I(x+i, y+j) < I(x, y): 62 bits, in any order.
 *   2. Every pixel is inside (no block margin).  Candidates of (x, y): d in [0, dmax(x)], dmax(x) = min(D - 1, x).
 *   3. Cost C(x, y, d) = popcount(cen_L(x, y) xor cen_R(x - d, y)) <= 62.
 *   4. Paths: the directions r are (+-1, 0) and (0, +-1), with paths = 8 also (+-1, +-1).  If the pixel p - r is outside the
 *      image, L_r(p, d) = C(p, d).  Otherwise, with M = the minimum of L_r(p - r, k) over the candidates k of p - r,
 *        L_r(p, d) = C(p, d) + min(L_r(p-r, d), L_r(p-r, d-1) + P1, L_r(p-r, d+1) + P1, M + P2) - M,
 *      terms whose disparity is not a candidate of p - r left out (M + P2 is always there).  So L_r <= 62 + P2 <= 254.
 *   5. S(p, d) = sum over r of L_r(p, d) <= 8 * 254 (fits 16 bits).
 *   6. Selection, steps 4 and 6-9 of the block matcher with S in place of C and no texture test: d* = the smallest minimiser of
 *      S over the candidates, S* = S(d*); uniqueness (u > 0): thr = S* + (S* u) / 100, invalid if a candidate with
 *      |d - d*| > 1 has S(d) <= thr; V-fit when 0 < d* < dmax(x): p = S(d*+1), n = S(d*-1), k = p + n - 2 S* + |p - n|,
 *      off = k ? ((n - p) 256) / k : 0 (C division), disp16 = (256 d* + off + 8) >> 4; left-right check (m >= 0): dR(xr, y) = the
 *      smallest d in [0, D-1] with xr + d < cols that minimises S(xr + d, y, d), over every pixel, valid or not; invalid if
 *      |dR(x - d*, y) - d*| > m.  Output int16 [rows][cols]: disp16, or VISO_DISP_INVALID.
 * Out of scope: a negative minimum disparity, OpenCV's SGBM cost (Birchfield-Tomasi), more than 8 paths.  The speckle filter is a
 * stage of its own (the next section).
 * HIP kernels (sgm.hip): census words, one launch per path direction over S [rows][cols][D] u16 in device memory, one selection
 * launch.  This build handles cols <= 2048 (VISO_ERR_UNSUPPORTED beyond). */
typedef struct viso_sgm_params {
    int32_t num_disp;      /* D */
    int32_t p1;            /* P1 */
    int32_t p2;            /* P2 */
    int32_t paths;         /* 4 or 8 */
    int32_t uniqueness;    /* u, percent */
    int32_t lr_max_diff;   /* m; -1 turns the left-right check off */
} viso_sgm_params;

/* D = 128, P1 = 10, P2 = 120, paths = 8, u = 10, m = 1.  Host only. */
void viso_sgm_params_default(viso_sgm_params* p);
/* Host pointers, default context: the map of one pair (out rows x cols int16).  The arguments are checked before any device is
 * touched: VISO_ERR_ARG for null pointers, sizes <= 0 or invalid parameters; VISO_ERR_UNSUPPORTED for cols > 2048; VISO_ERR_NOMEM
 * when the workspace cap cannot hold one frame. */
int viso_stereo_sgm(const uint8_t* left, const uint8_t* right, int rows, int cols, const viso_sgm_params* params, int16_t* out);
/* Turn SGM on with a copy of *params (off with NULL, the default): the batch's dense stage (viso_batch_run_images, also with
 * matcher_only, and viso_batch_run_disparity) then computes its maps with SGM, at the place and with the guarantees of
 * viso_batch_set_disparity; viso_batch_run_disparity and viso_batch_get_disparity(ies) serve them.  A batch has one map buffer, so
 * one method at a time: VISO_ERR_ARG while viso_batch_set_disparity is on (and viso_batch_set_disparity returns VISO_ERR_ARG while
 * SGM is on); the batch stays usable.  Descriptor-in runs return VISO_ERR_ARG while it is on.  The frames are processed in groups
 * whose census words and S volumes (rows cols (16 + 2 D) bytes a frame) fit the workspace cap; the workspace is allocated by the
 * first launch and freed with the batch, and the maps are the same for every group size.  A run returns VISO_ERR_NOMEM when the cap
 * cannot hold one frame.  VISO_ERR_ARG: invalid parameters, a dead handle. */
int viso_batch_set_sgm(viso_batch* b, const viso_sgm_params* params);
/* The workspace cap in bytes of every later SGM launch of the process (0: the default, 2 GiB). */
void viso_sgm_set_workspace_cap(size_t bytes);

/* ------------------------------------------------ speckle filter and 3-D reprojection of the maps (opt-in; NOT in the reference)
 *
 * The last stage of both methods above, in the form of OpenCV's filterSpeckles with newVal = the invalid value.  Parity with OpenCV
 * is not pinned (it is not a dependency); this definition is the contract, and the device output is bit-identical to it (it is
 * stated through components, so it depends on no traversal order).
 * Input: an int16 map [rows][cols] in the format above (1/16 px, VISO_DISP_INVALID for invalid).  Parameters S = max_size >= 0
 * (pixels) and Delta = max_diff in 0..4096 (map units, 1/16 px; 4096 is 256 px).  Any other value gives VISO_ERR_ARG.
 *   1. Pixels equal to VISO_DISP_INVALID belong to no component and stay as they are.
 *   2. Two valid pixels that are 4-neighbours are linked when |d(p) - d(q)| <= Delta.  The relation is symmetric.
 *   3. The components are the connected components of that graph over the whole image (not per tile, not per row).
 *   4. Every pixel of a component with at most S pixels becomes VISO_DISP_INVALID.  Every other pixel keeps its value.
 * S = 0 changes nothing and is valid (nothing is launched).
 * Out of scope: 8-connectivity, a median or hole-filling filter.
 * HIP kernels (speckle.hip): union-find over linear pixel indices: 64 x 16 tiles in LDS, the tile borders joined in device memory
 * by atomicMin on the larger root, a flatten-and-count pass (integer atomics, one per tile and component), the removal.  Four
 * launches for all frames of a group; no launch count or pass count depends on the shape of a component.  Workspace: 8 bytes a
 * pixel.  This build handles cols <= 2048 and rows cols < 2^31 (VISO_ERR_UNSUPPORTED beyond). */
typedef struct viso_speckle_params {
    int32_t max_size;   /* S, pixels */
    int32_t max_diff;   /* Delta, 1/16 px */
} viso_speckle_params;

/* S = 100, Delta = 16 (1 px).  Host only. */
void viso_speckle_params_default(viso_speckle_params* p);
/* Host pointer, default context, in place.  The arguments are checked before any device is touched: VISO_ERR_ARG for a null map,
 * sizes <= 0 or invalid parameters; VISO_ERR_UNSUPPORTED for cols > 2048; VISO_ERR_NOMEM when the workspace cap cannot hold one
 * frame. */
int viso_filter_speckles(int16_t* map, int rows, int cols, const viso_speckle_params* params);
/* Turn the filter on with a copy of *params (off with NULL, the default).  While on, the batch's dense stage
 * (viso_batch_run_images, also with matcher_only, and viso_batch_run_disparity) filters its map buffer in place right after the
 * method's last kernel, for block matching and for SGM alike, and viso_batch_get_disparity(ies) serve the filtered maps; every other
 * output is unchanged, and it stays outside the run's time stamps.  It may be set while no method is on: it then does nothing until
 * one is.  With it off nothing new is launched or allocated.  The frames are processed in groups whose label and size words fit the
 * workspace cap; the workspace is allocated by the first launch and freed with the batch, and the maps are the same for every group
 * size.  A run returns VISO_ERR_NOMEM when the cap cannot hold one frame, and the batch stays usable.  VISO_ERR_ARG: invalid
 * parameters, a dead handle. */
int viso_batch_set_speckle(viso_batch* b, const viso_speckle_params* params);
/* The workspace cap in bytes of every later speckle launch of the process (0: the default, 2 GiB). */
void viso_speckle_set_workspace_cap(size_t bytes);

/* Reprojection of a map to an organised point image out [rows][cols][3] float32 (the form of OpenCV's reprojectImageTo3D), with
 * the calibration f, cu, cv, base of *param and an optional pose T (4 x 4 row-major double, the first three rows are read; NULL =
 * identity, applied as no transform at all):
 *   - a pixel (x, y) is used when disp16 != VISO_DISP_INVALID and disp16 >= min_disp16 (min_disp16 >= 1, so a disparity of 0 never
 *     divides); every other pixel gets three NaNs;
 *   - in double: d = disp16 / 16, X = base (x - cu) / d, Y = base (y - cv) / d, Z = f base / d (the products first, then the
 *     division: the operand order of the sparse triangulation);
 *   - with a pose: P_i = ((T[i][0] X + T[i][1] Y) + T[i][2] Z) + T[i][3], i = 0..2, in double, in exactly that association, with
 *     no fused multiply-add;
 *   - then each coordinate is rounded once to float32.
 * Host pointers, default context; the arguments are checked before any device is touched (VISO_ERR_ARG: a null map, calibration or
 * output, sizes <= 0, min_disp16 < 1). */
int viso_disparity_to_points(const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_or_null,
                             int min_disp16, float* out);
/* The same over frame t's resident map of the batch (the filtered one while the speckle filter is on), with the calibration of
 * viso_batch_set_params: the kernel is launched on demand and the points copied out; the batch keeps no point buffer.
 * (viso_batch_get_points, the older call above, returns the solver's sparse inputs; hence the longer name.)  VISO_ERR_ARG when
 * disparity is off, no run has computed it, or the batch's parameters are not set. */
int viso_batch_get_disparity_points(viso_batch* b, int t, const double* pose_or_null, int min_disp16, float* out);

/* ------------------------------------------------ voxel map: dense maps and poses fused on the device (opt-in; NOT in the reference)
 *
 * A persistent hash table of voxels on the device that takes any number of (disparity map, pose) pairs and gives back a compact,
 * sorted list of the occupied voxels with observation counts and centroids.  Everything behind one double division is integer
 * arithmetic, so a map depends on neither the order of the frames nor on scheduling, and maps are additive: fusing a sequence in
 * any partition and adding the parts (viso_map_add_entries) gives the same bytes.  This definition is the contract; the device
 * output is bit-identical to tests/map_ref.py.
 * Parameters: voxel > 0 and finite (metres), min_disp16 >= 1 (1/16 px), capacity_log2 in 10..28 (the table has 2^capacity_log2
 * slots).  Any other value gives VISO_ERR_ARG.  s = voxel / 1024, computed once in double on the host, is the only derived constant.
 *   1. A pixel (x, y) of a frame contributes when disp16 != VISO_DISP_INVALID and disp16 >= min_disp16.
 *   2. Its world point P is the reprojection above in double, BEFORE that section's rounding to float32: d = disp16 / 16,
 *      X = base (x - cu) / d, Y = base (y - cv) / d, Z = f base / d, and with a pose P_i = ((T[i][0] X + T[i][1] Y) + T[i][2] Z) +
 *      T[i][3] in exactly that association, with no fused multiply-add; without one P = (X, Y, Z).  The pose is a 4 x 4 row-major
 *      matrix whose first three rows are read; all 16 entries must be finite (VISO_ERR_ARG, checked before any device is touched).
 *   3. Cell: g_i = (int64) floor(P_i / s), i = x, y, z: one IEEE double division and one floor.  If any |g_i| >= 2^30 (or P_i / s
 *      is not finite) the point is not inserted and n_out_of_range is incremented.
 *   4. Otherwise the voxel is k_i = g_i >> 10 (arithmetic shift: -2^20 <= k_i < 2^20) and the offset o_i = g_i & 1023.
 *      key = ((k_x + 2^20) << 42) | ((k_y + 2^20) << 21) | (k_z + 2^20): 63 bits; all ones marks an empty slot.
 *   5. Per voxel: count (uint32) += 1, sum[i] (uint64) += o_i.
 *   6. Extraction: every occupied voxel with count >= min_count (>= 1) as a viso_map_entry, sorted by key, ascending.
 *   7. Centroid of an entry (host only): c_i = (float)(((double)(k_i * 1024) + (double)sum[i] / (double)count + 0.5) * s).
 * Full table: insertion is open addressing (linear probing from a hash of the key) with a 64-bit compare-and-swap on the key array;
 * the probe loop is bounded by the capacity and advances strictly, so a full table is a wrong count, never a hang.  A point that
 * finds no slot increments n_dropped; a call that ends with n_dropped > 0 returns VISO_ERR_NOMEM and marks the map overflowed
 * (which points were dropped depends on scheduling), and viso_map_count / viso_map_get / viso_map_add_entries / the fuse calls
 * then refuse with VISO_ERR_NOMEM until viso_map_clear, after which the map is fully usable again.
 * Out of scope: RGB (a TSDF map can carry one 8-bit intensity: "TSDF intensity" below), fusing inside the KITTI runners while their chunks drain (a surface form is the
 * TSDF map below).
 * HIP kernels (voxelmap.hip): map_fuse_kernel (one thread per pixel of a group of frames; lanes that continue the key of the lane
 * to their left form a run, the run heads come from one ballot, the runs' sums from a wave scan, and only a run's head probes the
 * table and issues the four integer atomic adds); adding entries, listing and clearing are the kernels every table of voxels shares
 * (voxel_hash.h: voxel_add_entries_kernel, voxel_compact_kernel, voxel_clear_kernel, over the map's payload).  Memory: 36 bytes a
 * slot (604 MB at the default capacity). */
typedef struct viso_map_params {
    double voxel;            /* edge of a voxel, metres */
    int32_t min_disp16;      /* smallest disparity used, 1/16 px */
    int32_t capacity_log2;   /* log2 of the table's slots */
} viso_map_params;

typedef struct viso_map_entry {   /* 40 bytes */
    int32_t k[3];            /* voxel index: the voxel is [k voxel, (k + 1) voxel) on every axis */
    uint32_t count;          /* points fused into it */
    uint64_t sum[3];         /* sums of the points' offsets inside the voxel, in units of s = voxel / 1024 */
} viso_map_entry;

typedef struct viso_map_counters {
    uint64_t n_points;       /* pixels that contributed (step 1), the counts of added entries included */
    uint64_t n_inserts;      /* table insertions issued, after the combining inside the waves (a diagnostic: depends on the launch shape) */
    uint64_t n_out_of_range; /* step 3 */
    uint64_t n_dropped;      /* points that found no slot */
    uint64_t n_occupied;     /* slots in use */
} viso_map_counters;

typedef struct viso_map viso_map;

/* voxel 0.2, min_disp16 16 (1 px), capacity_log2 24.  Host only. */
void viso_map_params_default(viso_map_params* p);
/* A map on the context's device and stream (NULL: the default context), empty.  The arguments are checked before any device is
 * touched (VISO_ERR_ARG); VISO_ERR_NOMEM when the table cannot be allocated. */
int viso_map_create(viso_ctx* ctx_or_null, const viso_map_params* params, viso_map** out);
/* Frees the map.  VISO_OK also for a map whose context was destroyed before it (its memory is freed all the same); every other
 * call on such a map returns VISO_ERR_ARG, and so does anything on a handle that is not, or no longer, a map. */
int viso_map_destroy(viso_map* m);
/* Empties the table, zeroes the statistics and lifts the overflow mark. */
int viso_map_clear(viso_map* m);
/* Fuses one host map with the calibration f, cu, cv, base of *param (all finite) and the pose (NULL: no transform). */
int viso_map_fuse(viso_map* m, const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_or_null);
/* Fuses the resident maps of frames t0 .. t1-1 of the batch (the filtered ones while the speckle filter is on) with the calibration of
 * viso_batch_set_params and poses [t1 - t0][16], frame t0 + i with pose i, with no host copy of the maps.  The map and the batch must
 * share a context.  VISO_ERR_ARG when disparity is off, no run has computed it, or the batch's parameters are not set. */
int viso_batch_fuse_disparities(viso_batch* b, viso_map* m, int t0, int t1, const double* poses);
/* Adds n entries (of viso_map_get, of this or another map with the same voxel) to the table: count += count, sum += sum per voxel.
 * VISO_ERR_ARG: a k outside -2^20 .. 2^20 - 1, a count of 0, a sum[i] > 1023 count. */
int viso_map_add_entries(viso_map* m, const viso_map_entry* entries, size_t n);
/* The number of voxels with count >= min_count (>= 1). */
int viso_map_count(viso_map* m, uint32_t min_count, size_t* n);
/* Those voxels, sorted by key; *n = their number.  VISO_ERR_ARG, with *n set and nothing written, when n_cap is smaller.  The table is
 * compacted on the device; the sort runs on the host. */
int viso_map_get(viso_map* m, uint32_t min_count, viso_map_entry* entries_out, size_t n_cap, size_t* n);
int viso_map_stats(viso_map* m, viso_map_counters* out);
/* Step 7.  Host only; VISO_ERR_ARG for a null pointer, a count of 0, a voxel that is not finite and > 0. */
int viso_map_entry_centroid(const viso_map_entry* entry, double voxel, float out[3]);

/* ------------------------------------------------ TSDF map: signed-distance fusion and surface points (opt-in; NOT in the reference)
 *
 * A second persistent hash table of voxels on the device, beside the voxel map above and with its key, probe, full-table rule and
 * lifetime rules.  Where the voxel map counts the points that fall into a voxel, this one averages, per voxel, the signed distance
 * of the voxel's centre from the measured surface along the viewing direction, truncated to a band of T voxels (a truncated signed
 * distance function, TSDF); the surface is where the average changes sign between two neighbouring voxels.  Sum of distances and
 * sum of weights are integers, so a map depends on neither the order of the frames nor on scheduling, and maps are additive.  This
 * definition is the contract; the device output is bit-identical to tests/tsdf_ref.py.
 * Parameters: voxel > 0 and finite (metres), trunc_voxels T in 1..8, min_disp16 >= 1 (1/16 px), capacity_log2 in 10..28.  Any other
 * value gives VISO_ERR_ARG before a device is touched.  Derived once in double on the host: s = voxel / 1024 and h = voxel * 0.5.
 * Everything below is IEEE double in the operand order written, with no fused multiply-add.
 *   1. A pixel (x, y) of a frame contributes when disp16 != VISO_DISP_INVALID and disp16 >= min_disp16 (the voxel map's rule 1).
 *   2. Camera point: d = disp16 / 16, X = base (x - cu) / d, Y = base (y - cv) / d, Z = f base / d.
 *   3. Samples: for j = -2T .. +2T in ascending order, zj = Z + (double)j h.  A sample with !(zj > 0) is not inserted and resets
 *      the duplicate rule of step 5.  Otherwise r = zj / Z, Qc = (X r, Y r, zj), and the world point is
 *      Q_i = ((T[i][0] Qc0 + T[i][1] Qc1) + T[i][2] Qc2) + T[i][3].  The pose is a 4 x 4 row-major matrix whose 16 entries must be
 *      finite (VISO_ERR_ARG, checked before any device is touched); it is taken as rigid.  A null pose means Q = Qc.
 *   4. Grid cell: g_i = floor(Q_i / s).  Any |g_i| >= 2^30, or a quotient that is not finite: the sample is not inserted, counts in
 *      n_out_of_range and resets the duplicate rule.  Voxel k_i = g_i >> 10 (arithmetic shift); the key is the voxel map's.
 *   5. One update per pixel and voxel: a sample whose voxel equals that of the previous inserted sample of the same pixel is
 *      skipped (the ray is straight and voxels are convex, so equal voxels are consecutive).
 *   6. Projective distance of the voxel centre: C_i = (double)(k_i 1024 + 512) s,
 *      zc = (T[0][2] (C0 - T[0][3]) + T[1][2] (C1 - T[1][3])) + T[2][2] (C2 - T[2][3]), or zc = C2 without a pose, and
 *      q = (int64) floor((Z - zc) / s).  !(q >= -T 1024) (the voxel lies behind the surface by more than the truncation, or the
 *      quotient is not a number): no update, but the sample still is the previous sample of rule 5.  q > T 1024: q = T 1024.
 *   7. Per voxel: weight (uint32) += 1, sum (int64) += q.
 *   8. Voxels: viso_tsdf_get returns those with weight >= min_weight (>= 1), sorted by key, ascending.
 *   9. Surface crossings: for every voxel a with weight >= min_weight and axis = 0, 1, 2, let b = a + e_axis.  If b is in the table
 *      with weight >= min_weight and (sum_a < 0) != (sum_b < 0), a viso_tsdf_crossing is emitted.  Sorted by (key of a, axis).
 *  10. Crossing point (host only): da = (double)sa / (double)wa, db likewise, t = da / (da - db), and
 *      p_i = (float)(((double)(k_i 1024 + 512) + (i == axis ? t 1024.0 : 0.0)) s).
 * Full table: the voxel map's rule.  An update that finds no slot counts in n_dropped; a call that ends with n_dropped > 0 returns
 * VISO_ERR_NOMEM and marks the map overflowed, and every getter, viso_tsdf_add_entries and every fuse call then refuse with
 * VISO_ERR_NOMEM until viso_tsdf_clear.  Every probe loop, the read-only lookups of the extraction included, visits each slot at
 * most once and advances strictly.
 * Out of scope: RGB (one 8-bit intensity: "TSDF intensity" below), fusing inside the KITTI runners, the sort on the device.  (Carving
 * free space beyond the truncation band and weights that fall with depth: "TSDF fuse options" below.)
 * HIP kernels (tsdf.hip): tsdf_fuse_kernel (one thread per pixel of a group of frames; the loop over j is uniform across the wave,
 * and per j the lanes that continue the voxel of the lane to their left form a run whose head lane alone probes the table and
 * issues the two integer atomic adds), tsdf_crossings_kernel; adding entries, listing and clearing are the kernels every table of
 * voxels shares (voxel_hash.h: voxel_add_entries_kernel, voxel_compact_kernel, voxel_clear_kernel, over the TSDF map's payload).
 * Memory: 20 bytes a slot (1.34 GB at the default capacity). */
typedef struct viso_tsdf_params {
    double voxel;            /* edge of a voxel, metres */
    int32_t trunc_voxels;    /* T: the truncation band, in voxels */
    int32_t min_disp16;      /* smallest disparity used, 1/16 px */
    int32_t capacity_log2;   /* log2 of the table's slots */
} viso_tsdf_params;

typedef struct viso_tsdf_entry {   /* 24 bytes */
    int32_t k[3];            /* voxel index: the voxel is [k voxel, (k + 1) voxel) on every axis */
    uint32_t weight;         /* updates fused into it */
    int64_t sum;             /* sum of their q, in units of s = voxel / 1024; positive: the centre is in front of the surface */
} viso_tsdf_entry;

typedef struct viso_tsdf_crossing {   /* 40 bytes */
    int32_t k[3];            /* voxel a; b = a + e_axis */
    int32_t axis;
    uint32_t wa, wb;         /* weights of a and b */
    int64_t sa, sb;          /* sums of a and b */
} viso_tsdf_crossing;

typedef struct viso_tsdf_counters {
    uint64_t n_points;       /* pixels that contributed (step 1) */
    uint64_t n_updates;      /* updates of step 7, the weights of added entries included */
    uint64_t n_out_of_range; /* samples of step 4 */
    uint64_t n_dropped;      /* updates that found no slot */
    uint64_t n_occupied;     /* slots in use */
} viso_tsdf_counters;

typedef struct viso_tsdf viso_tsdf;

/* voxel 0.2, trunc_voxels 3, min_disp16 16 (1 px), capacity_log2 26.  Host only. */
void viso_tsdf_params_default(viso_tsdf_params* p);
/* A TSDF map on the context's device and stream (NULL: the default context), empty.  VISO_ERR_NOMEM when the table cannot be
 * allocated.  Handles follow the rules of viso_map: viso_tsdf_destroy frees the map and returns VISO_OK also when its context was
 * destroyed before it; every other call on such a map, or on a handle that is not a TSDF map, returns VISO_ERR_ARG. */
int viso_tsdf_create(viso_ctx* ctx_or_null, const viso_tsdf_params* params, viso_tsdf** out);
int viso_tsdf_destroy(viso_tsdf* t);
/* Empties the table, zeroes the statistics and lifts the overflow mark. */
int viso_tsdf_clear(viso_tsdf* t);
/* Fuses one host map with the calibration f, cu, cv, base of *param (all finite) and the pose (NULL: no transform). */
int viso_tsdf_fuse(viso_tsdf* t, const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_or_null);
/* Fuses the resident maps of frames t0 .. t1-1 of the batch, as viso_batch_fuse_disparities does and with its refusals. */
int viso_batch_fuse_tsdf(viso_batch* b, viso_tsdf* t, int t0, int t1, const double* poses);
/* Adds n entries (of viso_tsdf_get, of a map with the same voxel and truncation): weight += weight, sum += sum per voxel.
 * VISO_ERR_ARG: a k outside -2^20 .. 2^20 - 1, a weight of 0, |sum| > T 1024 weight. */
int viso_tsdf_add_entries(viso_tsdf* t, const viso_tsdf_entry* entries, size_t n);
/* Step 8: the number of voxels with weight >= min_weight, and those voxels (VISO_ERR_ARG, with *n set and nothing written, when
 * n_cap is smaller).  The table is compacted on the device; the sort runs on the host. */
int viso_tsdf_count(viso_tsdf* t, uint32_t min_weight, size_t* n);
int viso_tsdf_get(viso_tsdf* t, uint32_t min_weight, viso_tsdf_entry* entries_out, size_t n_cap, size_t* n);
/* Step 9, in the same two forms. */
int viso_tsdf_surface_count(viso_tsdf* t, uint32_t min_weight, size_t* n);
int viso_tsdf_surface(viso_tsdf* t, uint32_t min_weight, viso_tsdf_crossing* crossings_out, size_t n_cap, size_t* n);
int viso_tsdf_stats(viso_tsdf* t, viso_tsdf_counters* out);
/* Step 10.  Host only; VISO_ERR_ARG for a null pointer, an axis outside 0..2, a weight of 0, sums of the same sign, a voxel that
 * is not finite and > 0. */
int viso_tsdf_crossing_point(const viso_tsdf_crossing* crossing, double voxel, float out[3]);

/* ------------------------------------------------ TSDF fuse options: free-space carving and disparity-based weights (opt-in; NOT in
 * the reference)
 *
 * A TSDF map, plain or gray, carries fuse options that every way of fusing into it obeys (viso_tsdf_fuse, viso_tsdf_fuse_gray,
 * viso_batch_fuse_tsdf).  At their defaults every rule and every output above is unchanged, bit for bit, and the same kernels are
 * launched.  With them a frame also lowers the model where it looks through it, and a near measurement counts for more than a far
 * one.  Sums stay integers, so the map still depends on neither the order of the frames nor on scheduling, maps fused with the
 * same options are additive, and the device output is bit-identical to tests/carve_ref.py.
 * Options (four scalars of viso_tsdf_set_fuse_options; the header defines no struct for them): carve_voxels C in 0..1024, weight_shift
 * in -1..30, weight_max in 1..255 (read only when weight_shift >= 0), carve_near finite and >= 0 (metres).  Any other value gives VISO_ERR_ARG with the map's options unchanged, before a device is
 * touched.  The changes to the rules of "TSDF map"; nothing else changes:
 *   3. j runs over -(2T + 2C) .. +2T, ascending.  A sample with j < -2T is a free-space sample.  A free-space sample with
 *      zj < carve_near is not inserted and resets the duplicate rule of step 5, like one with !(zj > 0).  Steps 4, 5 and 6 apply to
 *      free-space samples unchanged: their q comes out clamped to T 1024 wherever the voxel's centre is more than the truncation in
 *      front of the point, by step 6 alone.
 *   7. The pixel's weight: w = 1 when weight_shift < 0, otherwise w = min(max((uint32)(disp16 disp16) >> weight_shift, 1), weight_max)
 *      with the pixel's own disp16: integer, and proportional to 1 / Z^2 between the clamps (stereo depth error grows with Z^2).
 *      Per voxel: weight += w, sum += w q; on a gray map gray += w I.  All of a pixel's samples carry its w, free-space ones
 *      included.
 * Counters: n_updates and n_dropped count updates, not weights.  |sum| <= T 1024 weight and gray <= 255 weight hold as before, so
 * viso_tsdf_add_entries and viso_tsdf_add_gray_entries take such a map's entries.
 * min_weight: with weights on, the thresholds of viso_tsdf_get, viso_tsdf_count, viso_tsdf_surface, viso_tsdf_mesh, viso_tsdf_render
 * and the align calls compare sums of w, no longer numbers of observations.
 * The 32-bit weight: one frame cannot wrap it (rows cols 255 < 2^32 for every accepted shape).  Many frames can, with carving, in the
 * voxels close to a camera that stands still, because every ray passes through them; carve_near is there to leave those out.  A
 * voxel that takes a free-space update holds a sample at depth >= carve_near, so every sample inside it lies at depth
 * >= z0 = carve_near - sqrt(3) voxel; for z0 > 0 the pixels that update it span at most f sqrt(3) voxel (1 + t) / z0 + 1 columns and
 * as many rows, t the largest |x - cu| / f, |y - cv| / f of the image, and a pixel updates a voxel once.  So one frame adds to such
 * a voxel at most  weight_max (f sqrt(3) voxel (1 + t) / (carve_near - sqrt(3) voxel) + 1)^2  (weight_max = 1 without weights), and
 * never more than rows cols weight_max.  The library does not detect a wrapped weight; tests/carve_ref.py asserts that none occurs.
 * Out of scope: carving only voxels that exist already (cheaper, but dependent on the frames' order), a lower weight for free-space
 * samples, eviction by weight, detecting a wrapped weight on the device.
 * HIP kernels (tsdf.hip): tsdf_carve_fuse_kernel and tsdf_gray_carve_fuse_kernel, the fuse kernels' body with the pixel's weight
 * carried: the loop over j stays uniform across the wave and starts at the smallest j at which a lane of the wave has a sample to
 * insert; a run's sums of w, w q and w I come from wave scans, and only its head lane probes the table. */
/* Sets the four options of a plain or gray map for every later fuse; they persist across viso_tsdf_clear.  A new map has
 * carve_voxels 0, weight_shift -1, weight_max 255, carve_near 0: the map of "TSDF map".  The values are checked first, then the
 * handle.  Changing them on a map that is not empty mixes frames fused by different rules: the map stays valid, but is no longer
 * the restatement of one option set.
 *   carve_voxels   C: 0 (off) .. 1024: voxels in front of the band that a pixel's ray also updates
 *   weight_shift   -1 (off): every update weighs 1; 0 .. 30
 *   weight_max     1 .. 255; read (and checked) only when weight_shift >= 0
 *   carve_near     metres, finite, >= 0: free-space samples nearer than this are not inserted */
int viso_tsdf_set_fuse_options(viso_tsdf* t, int32_t carve_voxels, int32_t weight_shift, uint32_t weight_max, double carve_near);
/* The map's options as they were set; all four outputs non-null. */
int viso_tsdf_get_fuse_options(viso_tsdf* t, int32_t* carve_voxels, int32_t* weight_shift, uint32_t* weight_max, double* carve_near);

/* ------------------------------------------------ TSDF mesh: triangles by marching tetrahedra (opt-in; NOT in the reference)
 *
 * The surface of a TSDF map as a triangle mesh.  A mesh is a function of the signs and the integer sums of the voxels alone, so it
 * depends on neither the order of the frames nor on scheduling.  This definition is the contract; the device output is
 * bit-identical to tests/mesh_ref.py.  Marching tetrahedra rather than marching cubes: the 16 cases of one tetrahedron follow from
 * the rule below, no face is ambiguous, and the subdivision is the same in every cube and matches across cube faces, so the mesh is
 * a closed oriented 2-manifold wherever the data is complete.
 *   Voxels: a voxel is usable when weight >= min_weight (min_weight >= 1).  A usable voxel is negative when sum < 0, otherwise
 *     positive (the rule of step 9 above).
 *   Cells: the cell of voxel k has the 8 corners k + (dx, dy, dz), dx, dy, dz in {0, 1}.  A cell with a corner that is not usable
 *     emits nothing.  A cell with k_i = 2^20 - 1 on any axis emits nothing: no key is formed beyond a field.
 *   Tetrahedra: the six permutations pi of (0, 1, 2) in lexicographic order are the tetrahedra 0..5 of a cell, with the corners
 *     c0 = k, c1 = c0 + e_pi0, c2 = c1 + e_pi1, c3 = c2 + e_pi2 = k + (1, 1, 1) (the Kuhn subdivision).
 *   Edges: the edge between ci and cj (i < j) belongs to voxel ci; its direction is d = cj - ci in {0, 1}^3 \ 0, with the code
 *     dir = dx + 2 dy + 4 dz (1..7; the axes are 1, 2, 4).  Edge (a, dir) carries a vertex when both ends a and b = a + d are usable
 *     and differ in sign.  With da = (double)sa / (double)wa, db likewise, t = da / (da - db):
 *     p_i = (float)(((double)(a_i 1024 + 512) + (d_i ? t 1024.0 : 0.0)) s), s = voxel / 1024.  For dir = 1, 2, 4 this is step 10
 *     above bit for bit.  t lies in [0, 1); t = 0 when sum_a = 0, and the triangles of zero area that follow stay in the list.
 *   Triangles of a tetrahedron, N its negative and P its positive corners, each by ascending local index, e(i, j) the vertex on
 *     the edge between corners i and j: N or P empty: none.  One corner i alone on its side: (e(i, j1), e(i, j2), e(i, j3)) over
 *     the other corners ascending.  N = {a, b}, P = {c, d}: (e(a, c), e(a, d), e(b, d)) and (e(a, c), e(b, d), e(b, c)), index 0, 1.
 *   Orientation: the normal points to the positive side, towards the camera that saw the surface.  With every vertex at its edge
 *     midpoint (2 owner + d, in half voxels), n = (v1 - v0) x (v2 - v0) and g = |N| sum_P c - |P| sum_N c: v1 and v2 are swapped
 *     when n . g < 0 (n . g is never 0).  The interpolated triangle has the orientation of the midpoint one.
 *   Output: the vertices some triangle refers to, sorted by (key of owner, dir); the triangles as indices into that list, sorted
 *     by (key of cell, tetrahedron, index).  More than 2^32 - 1 vertices: VISO_ERR_UNSUPPORTED.
 * Full table, the overflowed state and the lifetime of the handle are the TSDF map's.
 * HIP kernel (tsdf.hip): tsdf_mesh_kernel, one thread per slot: seven read-only probes for the other corners of its cell; the
 * sign-changing edges it owns as vertex records, positions computed on the device in double, and, when all eight corners are
 * usable, the cell's at most 12 triangles as references (cell, tetrahedron, index, three (corner, dir)).  Count pass and list pass
 * as for the crossings.  An owned edge can belong to a complete cell other than its owner's, so every sign-changing edge is
 * emitted; the host sorts both lists, drops the vertices no triangle refers to and resolves the references by binary search. */
typedef struct viso_tsdf_mesh_vertex {   /* 32 bytes */
    int32_t k[3];            /* the edge's owner a; its other end is a + (dir & 1, dir >> 1 & 1, dir >> 2) */
    int32_t dir;             /* 1..7 */
    float p[3];              /* position, metres */
    uint32_t weight;         /* min(wa, wb) */
} viso_tsdf_mesh_vertex;

typedef struct viso_tsdf_triangle {   /* 12 bytes */
    uint32_t v[3];           /* indices into the vertex list */
} viso_tsdf_triangle;

/* The numbers of vertices and triangles of the mesh at min_weight.  (The whole extraction runs: which vertices are referred to is
 * only known once the references are resolved.) */
int viso_tsdf_mesh_count(viso_tsdf* t, uint32_t min_weight, size_t* n_vertices, size_t* n_triangles);
/* The mesh.  Arguments are checked before any device is touched, with the refusals of viso_tsdf_surface.  VISO_ERR_ARG, with both
 * numbers set and nothing written, when either capacity is smaller. */
int viso_tsdf_mesh(viso_tsdf* t, uint32_t min_weight, viso_tsdf_mesh_vertex* vertices_out, size_t nv_cap,
                   viso_tsdf_triangle* triangles_out, size_t nt_cap, size_t* n_vertices, size_t* n_triangles);

/* ------------------------------------------------ TSDF render: disparity maps of the map at any pose, by ray casting (opt-in; NOT
 * in the reference)
 *
 * What a camera at a pose would see of a TSDF map, as an ordinary int16 map in 1/16 px: it goes wherever a measured map goes
 * (viso_disparity_to_points, viso_filter_speckles, viso_map_fuse, the KITTI PNGs).  A render reads the table only: the table, its
 * statistics and the overflow mark are untouched.  This definition is the contract; the device output is bit-identical to
 * tests/render_ref.py.  Everything is IEEE double in the operand order written, with no fused multiply-add.
 * Inputs: the map; min_weight >= 1; a viso_param of which f, cu, cv, base are read (all finite, f > 0, base > 0); rows, cols >= 1
 * with rows cols <= 2^31 - 1; max_depth finite and > 0; n_views >= 1; poses [n_views][16], row-major 4 x 4, camera to world, as
 * viso_tsdf_fuse takes them, all entries finite, or NULL, which means no transform and only with n_views == 1.  s = voxel / 1024 and
 * h = voxel * 0.5 are the map's own; N = (int) floor(max_depth / h) must lie in 1 .. 65536.  Any violation: VISO_ERR_ARG before a
 * device is touched.
 * Per view and pixel (x, y):
 *   1. Ray: a = ((double)x - cu) / f, b = ((double)y - cv) / f.
 *   2. Samples i = 1 .. N ascending: z_i = (double)i h (not accumulated), Qc = (a z_i, b z_i, z_i), and the world point Q as step 3
 *      of the TSDF map forms it (((T[i][0] Qc0 + T[i][1] Qc1) + T[i][2] Qc2) + T[i][3]; no pose: Q = Qc).
 *   3. Voxel: g_i = floor(Q_i / s), k_i = g_i >> 10, as step 4 of the map.  Any |g_i| >= 2^30, or a quotient that is not finite:
 *      the sample is a gap.
 *   4. The ray's voxel sequence: a sample whose voxel equals the voxel of the previous non-gap sample is skipped.  A gap empties
 *      "previous".
 *   5. A voxel is usable when it is in the table with weight >= min_weight.  One that is not still becomes "previous" for rule 4,
 *      marked not usable.
 *   6. Hit: the first sample whose voxel b is usable with sum_b < 0 and whose previous voxel a (the element of the sequence right
 *      before it, with no gap between) is usable with sum_a >= 0.  Only crossings from the front to the back count: a surface seen
 *      from behind renders as nothing.  The ray ends at the hit.
 *   7. Depth of the hit: the centre depths za, zb of a and b in this view's camera by step 6 of the map (C_i = (double)(k_i 1024 +
 *      512) s, zc = (T[0][2] (C0 - T[0][3]) + T[1][2] (C1 - T[1][3])) + T[2][2] (C2 - T[2][3]); no pose: C2);
 *      da = (double)sa / (double)wa, db likewise, t = da / (da - db), zs = za + (zb - za) t.  For a fronto-parallel surface seen
 *      from the pose it was fused from, da s = Z - za and db s = Z - zb up to the floor of step 6, so zs = Z up to 2 s: that is why
 *      the interpolation runs over centre depths and not over sample positions.
 *   8. v = ((f base) / zs) 16.0 + 0.5.  !(zs > 0), !(v >= 1.0) or v >= 32768.0: the pixel is invalid.  Otherwise
 *      disp16 = (int16) floor(v) and weight = min(wa, wb).
 *   9. No hit within the N samples, or an invalid value: VISO_DISP_INVALID, weight 0.
 * The surface is looked up in the nearest voxel and the distances are projective (along the fusing views' axes), so a slanted
 * surface and a view away from the fusing poses come back within a few sixteenths of a pixel, and a depth edge bleeds by up to a
 * voxel's footprint (DESIGN.md 5.17 has the figures).
 * An overflowed map refuses with VISO_ERR_NOMEM, as the getters do; a handle that is not a live TSDF map, or whose context is gone,
 * VISO_ERR_ARG; no device, VISO_ERR_HIP.  The call takes the map's lock, like an extraction.
 * Out of scope: trilinear rendering (the distance is sampled trilinearly by "TSDF align" below), an
 * empty-space skipping structure (a coarse block table), rendering into a batch's resident maps, RGB (one 8-bit intensity: "TSDF
 * intensity" below).  Normals of the hits: "TSDF normals" below.  Frame-to-model alignment: "TSDF align" below.
 * HIP kernel (tsdf.hip): tsdf_render_kernel, one thread per pixel of a group of views, the lanes of a wave consecutive pixels of a
 * row.  The loop over i is uniform across the wave; per i the lanes that continue the voxel of the lane to their left form a run,
 * whose head lane alone probes the table and loads weight and sum, and the other lanes take them from it.  Reads only: no atomics,
 * no LDS, no scratch; the probe loop is bounded by the capacity and advances strictly. */
/* disp_out: [n_views][rows][cols]; weight_out_or_null: the same shape, or NULL.  The views go through a device buffer that is
 * freed on every path (VISO_ERR_NOMEM when it cannot be allocated). */
int viso_tsdf_render(viso_tsdf* t, uint32_t min_weight, const viso_param* param, int rows, int cols, double max_depth,
                     const double* poses_or_null, int n_views, int16_t* disp_out, uint32_t* weight_out_or_null);

/* ------------------------------------------------ TSDF intensity: the cameras' 8-bit intensity fused, meshed and rendered (opt-in;
 * NOT in the reference)
 *
 * A gray map is a TSDF map whose table carries a third payload array, gray [slots] u64: per voxel the sum of the 8-bit intensities
 * of the pixels that updated it.  The sums are integers, so a gray map too depends on neither the order of the frames nor on
 * scheduling, and gray maps are additive.  The images are grayscale: "colour" is one intensity.  This definition is the contract; the
 * device output is bit-identical to tests/gray_ref.py.  Everything is IEEE double in the operand order written, with no fused
 * multiply-add.  A plain map (viso_tsdf_create) keeps its 20 bytes a slot, its kernels and its outputs.
 * Gray map: viso_tsdf_create_gray is viso_tsdf_create with the same parameter checks; memory is 28 bytes a slot.  viso_tsdf_clear
 *   zeroes gray too; viso_tsdf_is_gray tells which kind a handle is.  Handles, lifetime, lock and the full-table rule are the TSDF
 *   map's.
 * Fuse: viso_tsdf_fuse_gray takes with the map the left image it was computed from, uint8 [rows][cols], pixel for pixel.  Rules
 *   1..7 of the TSDF map hold unchanged, and rule 7 gains one line: every update of pixel (x, y) also does gray += image[y][x].  A
 *   voxel's intensity weight is therefore its weight, gray <= 255 weight always, and (k, weight, sum) of a gray map equal those of
 *   a plain map fused from the same frames, bit for bit.
 * Resident path: viso_batch_fuse_tsdf given a gray map also reads the batch's resident left images, frame t's at
 *   images + (2 t) rows cols: the images the run read, rectified if rectification was on.  VISO_ERR_ARG when the images' geometry
 *   is not the maps'.  Given a plain map it is unchanged.
 * Kinds do not mix.  VISO_ERR_ARG before a device is touched, the table unchanged: viso_tsdf_fuse or viso_tsdf_add_entries on a
 *   gray map; viso_tsdf_fuse_gray, viso_tsdf_add_gray_entries, viso_tsdf_get_gray, viso_tsdf_vertex_gray or viso_tsdf_render_gray
 *   on a plain map; a null image.
 * Entries: viso_tsdf_get_gray lists viso_tsdf_gray_entry sorted by key, with the two passes of viso_tsdf_get (viso_tsdf_count
 *   serves both kinds); viso_tsdf_add_gray_entries applies the checks of viso_tsdf_add_entries and gray <= 255 weight.
 * The unchanged readers work on a gray map with unchanged output: viso_tsdf_get, _surface, _mesh, _render, _stats.
 * Intensity of a point on an edge (vertices and renders): voxels a and b with weights wa, wb >= 1, sums sa, sb of different sign
 *   ((sa < 0) != (sb < 0)) and gray sums ga, gb.  da = (double)sa / (double)wa, db likewise, t = da / (da - db): exactly the
 *   mesh's and the render's.  ia = (double)ga / (double)wa, ib likewise, v = ia + (ib - ia) t,
 *   g = (uint8) min(255.0, floor(v + 0.5)).
 * Vertices: viso_tsdf_vertex_gray, for the vertex list of viso_tsdf_mesh or any list of (k, dir) (p and weight are not read): a = k,
 *   b = a + (dir & 1, dir >> 1 & 1, dir >> 2).  VISO_ERR_ARG before a device is touched for a dir outside 1..7, a k outside the
 *   key range, or a k_i = 2^20 - 1 on an axis where dir has its bit set.  An end that is not in the table, or ends that do not
 *   differ in sign: g = 0, the vertex counts in *n_missing, and the call still returns VISO_OK.  Crossings go through the same call
 *   with dir = 1 << axis.
 * Render: viso_tsdf_render_gray has the arguments and checks of viso_tsdf_render, and its disp_out and weight_out are bit-identical
 *   to it on the same table.  gray_out is g of the hit, a the previous voxel of rule 6, b the hit voxel, t rule 7's; 0 wherever the
 *   pixel is VISO_DISP_INVALID.
 * Out of scope: RGB, intensity weights other than the TSDF weight, exposure compensation, trilinear intensity, fusing inside the
 * KITTI runners.
 * HIP kernels (tsdf.hip): tsdf_gray_fuse_kernel (the fuse kernel's march with the pixel's intensity carried: one byte a pixel read
 * along the row, the run's sum of intensities from a second wave scan, three integer atomic adds from the run's head lane),
 * tsdf_gray_sample_kernel (one thread per vertex, two read-only probes, n_missing with one atomic per wave),
 * tsdf_gray_render_kernel (the render march, the head lane also loads gray and hands it to its run); adding entries, listing and
 * clearing are the shared kernels of voxel_hash.h over the gray map's payload, which carries the third array.  No LDS, no scratch;
 * every probe loop is bounded by the capacity. */
typedef struct viso_tsdf_gray_entry {   /* 32 bytes */
    int32_t k[3];
    uint32_t weight;
    int64_t sum;
    uint64_t gray;           /* sum of the updates' intensities: gray / weight is the voxel's mean intensity */
} viso_tsdf_gray_entry;

int viso_tsdf_create_gray(viso_ctx* ctx_or_null, const viso_tsdf_params* params, viso_tsdf** out);
/* *out = 1 for a gray map, 0 for a plain one.  Host only. */
int viso_tsdf_is_gray(viso_tsdf* t, int* out);
/* image: uint8 [rows][cols], the left image of the pair the map was computed from. */
int viso_tsdf_fuse_gray(viso_tsdf* t, const int16_t* disp, const uint8_t* image, int rows, int cols, const viso_param* param,
                        const double* pose_or_null);
int viso_tsdf_get_gray(viso_tsdf* t, uint32_t min_weight, viso_tsdf_gray_entry* entries_out, size_t n_cap, size_t* n);
int viso_tsdf_add_gray_entries(viso_tsdf* t, const viso_tsdf_gray_entry* entries, size_t n);
/* gray_out: uint8 [n]; n_missing_or_null: the number of vertices without a value. */
int viso_tsdf_vertex_gray(viso_tsdf* t, const viso_tsdf_mesh_vertex* vertices, size_t n, uint8_t* gray_out, size_t* n_missing_or_null);
/* gray_out: uint8 [n_views][rows][cols]; it goes through the same device buffer as the other two outputs. */
int viso_tsdf_render_gray(viso_tsdf* t, uint32_t min_weight, const viso_param* param, int rows, int cols, double max_depth,
                          const double* poses_or_null, int n_views, int16_t* disp_out, uint32_t* weight_out_or_null, uint8_t* gray_out);

/* ------------------------------------------------ TSDF normals: which way the surface faces, at vertices, crossings and rendered
 * hits (opt-in; NOT in the reference)
 *
 * The gradient of the averaged signed distance over a voxel's six neighbours, interpolated along the edge on which the surface
 * point lies: the gradient of a function is perpendicular to its zero level set, and that holds for the projective distances of
 * the map too.  The calls read the table only (weight and sum: a plain and a gray map alike); the table, its statistics and the
 * overflow mark are untouched.  This definition is the contract; the device output is bit-identical to tests/normal_ref.py.
 * Everything is IEEE double in the operand order written, with no fused multiply-add; the outputs are the doubles cast to float.
 * Usable voxel: in the table with weight >= min_weight, min_weight >= 1.  For a usable voxel v, d(v) = (double)sum_v /
 *   (double)weight_v.
 * Gradient of a usable voxel v: per axis i, p = v + e_i and m = v - e_i; a neighbour whose index would leave the key range on that
 *   axis (k_i = 2^20 - 1 has no p, k_i = -2^20 no m) is not usable.  Both usable: G_i = (d(p) - d(m)) * 0.5.  Only p:
 *   G_i = d(p) - d(v).  Only m: G_i = d(v) - d(m).  Neither: v has no gradient.  v has a gradient only when all three axes have one.
 * Normal of a point on the edge (a, dir), b = a + (dir & 1, dir >> 1 & 1, dir >> 2): a and b usable with sums of different sign,
 *   (sa < 0) != (sb < 0), otherwise the normal is missing.  da = d(a), db = d(b), t = da / (da - db): exactly the mesh's and the
 *   render's.  Both ends must have a gradient, otherwise the normal is missing.  g_i = Ga_i + (Gb_i - Ga_i) * t,
 *   L = sqrt((g0 g0 + g1 g1) + g2 g2); !(L > 0) or L not finite: missing.  Otherwise n_i = g_i / L in double, and the output is
 *   (float)n_i.  A missing normal is (0, 0, 0).  The normal points to the positive side, towards the cameras that saw the surface:
 *   the orientation the mesh's triangles have.
 * Vertices and crossings: viso_tsdf_vertex_normals, for the vertex list of viso_tsdf_mesh or any list of (k, dir) (p and weight are
 *   not read), in the world frame.  VISO_ERR_ARG before a device is touched, whatever the handle: min_weight == 0, a null list or
 *   output with n > 0, a dir outside 1..7, a k outside the key range, a k_i = 2^20 - 1 on an axis where dir has its bit set.
 *   Missing normals are counted in *n_missing, and the call still returns VISO_OK.  Crossings go through the same call with
 *   dir = 1 << axis.
 * Render: viso_tsdf_render_normals has the arguments and checks of viso_tsdf_render plus a non-null normals_out, and its disp_out
 *   and weight_out are bit-identical to it on the same table.  At a valid pixel the normal is that of the hit: a the previous voxel
 *   of rule 6, b the hit voxel, t rule 7's (the two need not be axis neighbours; the definition does not ask for it).  It is rotated
 *   into the view's camera frame before the cast: nc_j = (T[0][j] n0 + T[1][j] n1) + T[2][j] n2; no pose: nc = n.  (0, 0, 0)
 *   wherever the pixel is VISO_DISP_INVALID and where the normal is missing.  normals_out is laid out like the points of
 *   viso_disparity_to_points of the same map without a pose, so the two pair up pixel for pixel.  Intensity and normals are not
 *   combined in one call: a gray map's viso_tsdf_render_gray gives the intensity of the same hits.
 * An overflowed map refuses with VISO_ERR_NOMEM; a handle that is not a live TSDF map, or whose context is gone, VISO_ERR_ARG; no
 * device, VISO_ERR_HIP.  The calls take the map's lock, like an extraction.
 * Limits: both ends of the edge need a gradient, so normals are missing along the rim of the data.  The distances are projective
 * (along the fusing views' axes), so the normal is exact only at the crossing and only up to the grid (DESIGN.md 5.23 has the
 * angles).  No smoothing is applied.
 * Out of scope: smoothed or area-weighted normals, trilinear rendering, a shading kernel on the device (shade_normals of the Python
 * package is numpy), normals in the batch, point-to-plane alignment.
 * HIP kernels (tsdf.hip): tsdf_normal_sample_kernel (one thread per vertex: two read-only probes for the ends, then at most ten
 * for the two gradients, n_missing with one ballot and one atomic per wave), tsdf_normal_render_kernel (the render march unchanged;
 * a lane keeps the two voxels of its hit and the at most twelve probes of the gradients run behind the march, where the wave is
 * converged).  No LDS, no scratch; every probe loop is bounded by the capacity. */
/* normals_out: float [n][3]; n_missing_or_null: the number of vertices without a normal. */
int viso_tsdf_vertex_normals(viso_tsdf* t, uint32_t min_weight, const viso_tsdf_mesh_vertex* vertices, size_t n, float* normals_out,
                             size_t* n_missing_or_null);
/* normals_out: float [n_views][rows][cols][3]; it goes through the same device buffer as the other two outputs. */
int viso_tsdf_render_normals(viso_tsdf* t, uint32_t min_weight, const viso_param* param, int rows, int cols, double max_depth,
                             const double* poses_or_null, int n_views, int16_t* disp_out, uint32_t* weight_out_or_null, float* normals_out);

/* ------------------------------------------------ TSDF align: the pose at which a measured map lies on the model (opt-in; NOT in
 * the reference)
 *
 * Frame-to-model alignment by direct tracking on the signed distance (Bylow, Sturm, Kerl, Kahl, Cremers: Real-time camera tracking
 * and 3D reconstruction using signed distance functions, RSS 2013): no ray cast and no search for correspondences.  Every valid
 * pixel of a measured disparity map is back-projected with a pose guess, samples the map's averaged signed distance trilinearly
 * and contributes one row to a 6 x 6 Gauss-Newton system; the solution moves the pose so that the points come to lie on the
 * distance's zero set.  The normal equations are sums of integers: per pixel the six entries of the row and the residual are formed
 * in double, rounded once to integers, and their 28 pairwise products are summed as int64.  The sums depend on neither the order
 * of the pixels nor on scheduling, and the device output is bit-identical to tests/align_ref.py.  This definition is the contract.
 * Everything is IEEE double in the operand order written, with no fused multiply-add.  A linearise and an align read the table
 * only: the table, its statistics and the overflow mark are untouched; a gray map is accepted, of which only weight and sum are read.
 * Parameters (viso_tsdf_align_params): min_weight >= 1; gate_voxels finite, 0 < gate_voxels <= the map's trunc_voxels; max_iters in
 * 1..50; eps_rot (rad) and eps_trans (m) finite and >= 0; min_pixels >= 6.
 * Inputs of a linearise: the map; disp int16 [rows][cols], rows, cols >= 1 and rows cols <= 2^22 (a product of two entries is below
 * 2^40, so a sum stays below 2^62); a viso_param of which f, cu, cv, base are read (all finite, f > 0, base > 0); one pose, 4 x 4
 * row-major, camera to world, as viso_tsdf_fuse takes it, its first three rows finite (the fourth is not read), taken as rigid, or
 * NULL: the identity matrix.  voxel and s = voxel / 1024 are the map's own, G = gate_voxels 1024.0.  Any violation: VISO_ERR_ARG;
 * the checks that do not need the map come before the handle is looked at.
 * Per pixel (x, y):
 *   1. It contributes by rules 1 and 2 of the TSDF map with the map's min_disp16: P = (X, Y, Z).  n_points += 1.
 *   2. World point: Q_i = ((T[i][0] X + T[i][1] Y) + T[i][2] Z) + T[i][3].
 *   3. u_i = Q_i / voxel - 0.5 (a voxel's centre has integer u), k0_i = floor(u_i), t_i = u_i - k0_i.  A u_i that is not finite,
 *      or a k0_i outside -2^20 .. 2^20 - 2: n_out_of_range += 1, the pixel is skipped.
 *   4. The eight voxels k0 + (dx, dy, dz), d in {0, 1}.  A voxel is usable when it is in the table with weight >= min_weight.  Any
 *      of the eight not usable: n_missing += 1, the pixel is skipped.  m[dz][dy][dx] = (double)sum / (double)weight.
 *   5. Along x, for the four (dy, dz):  X1[dz][dy] = m[dz][dy][1] - m[dz][dy][0],  X0[dz][dy] = m[dz][dy][0] + t_0 X1[dz][dy].
 *      Along y, for the two dz:         Y1[dz] = X0[dz][1] - X0[dz][0],             Y0[dz] = X0[dz][0] + t_1 Y1[dz],
 *                                       YX[dz] = X1[dz][0] + t_1 (X1[dz][1] - X1[dz][0]).
 *      Along z:  psi = Y0[0] + t_2 (Y0[1] - Y0[0]),  D0 = YX[0] + t_2 (YX[1] - YX[0]),  D1 = Y1[0] + t_2 (Y1[1] - Y1[0]),
 *                D2 = Y0[1] - Y0[0].  psi is the distance in units of s, D its derivative per voxel; g_i = D_i / 1024.0 is metres
 *      per metre.
 *   6. Gate: |psi| > G: n_gated += 1, the pixel is skipped.
 *   7. w = (f base) / (Z Z): the residual is in pixels of disparity, which whitens stereo's depth noise.  e = (psi s) w.
 *      The gradient in the camera: c_j = (T[0][j] g_0 + T[1][j] g_1) + T[2][j] g_2.  The row, for an increment on the camera's side
 *      (T <- T D(xi), xi = (v, omega): translation first), which keeps the system conditioned far from the world's origin:
 *      a_0..2 = c_j w;  a_3 = (Y c_2 - Z c_1) w,  a_4 = (Z c_0 - X c_2) w,  a_5 = (X c_1 - Y c_0) w   (P x c).
 *   8. A_i = floor(a_i 256.0 + 0.5) for i < 6, A_6 = floor(e 256.0 + 0.5).  A value that is not finite or |A_i| >= 2^20:
 *      n_clipped += 1, the pixel is skipped.
 *   9. n_used += 1, and for 0 <= i <= j <= 6: N[i][j] += A_i A_j (int64).  n[28] holds the upper triangle row by row:
 *      N[i][j] = n[7 i - i (i - 1) / 2 + (j - i)].
 * Align (viso_tsdf_align): on the host around the kernel, with T the guess (NULL: the identity) and its fourth row set to 0 0 0 1.
 *   For it = 0 .. max_iters - 1:
 *   a. Linearise at T.  H = N[:6][:6] / 65536.0 (both triangles), b_i = N[i][6] / 65536.0, C = N[6][6] / 65536.0.
 *   b. n_used < min_pixels: status -1.
 *   c. Cholesky H = L L', row by row: d = H[j][j] - L[j][0]^2 - .. - L[j][j-1]^2 (subtracted in that order); !(d > 1e-12 H[j][j]):
 *      status -2 (a single wall, for example, leaves three directions free); L[j][j] = sqrt(d),
 *      L[i][j] = (H[i][j] - L[i][0] L[j][0] - .. - L[i][j-1] L[j][j-1]) / L[j][j].
 *   d. xi = -(H^-1 b) by the two triangular solves.  An entry that is not finite: status -3.
 *   e. D(xi): theta2 = (omega_0^2 + omega_1^2) + omega_2^2, theta = sqrt(theta2); A = sin(theta) / theta and
 *      B = (1 - cos(theta)) / theta2, or for theta < 1e-8: A = 1 - theta2 / 6, B = 0.5 - theta2 / 24; with K the cross-product
 *      matrix of omega, R = I + A K + B (omega omega' - theta2 I), and D = [R v; 0 1].
 *      T[i][j] <- (T[i][0] D[0][j] + T[i][1] D[1][j]) + T[i][2] D[2][j], and for j = 3: that + T[i][3].  iters = it + 1.
 *   f. ||omega|| <= eps_rot and ||v|| <= eps_trans: status 1, the loop ends.  max_iters steps without that: status 2; the pose is
 *      returned all the same.
 *   One more linearise at the final T, with the checks b and c, gives cost = sqrt(C / n_used), n_used and
 *   cov = (C / max(n_used - 6, 1)) H^-1 in the (v, omega) order of the row.
 *   On a status < 0, pose is the guess and every other number of the record is zero.
 *   Trace: trace_out_or_null [trace_cap] receives one viso_tsdf_align_step per linearise in their order, the last one included
 *   (at most max_iters + 1; those beyond trace_cap are not recorded, entries that are not written are not touched; a written
 *   entry's pose ends in 0 0 0 1).
 * Resident path: viso_batch_align_tsdf aligns the batch's resident maps t0 .. t1-1, each on its own against the same model, with the
 * batch's calibration and with no host copy of the maps: records_out [t1 - t0], each what viso_tsdf_align gives for that map and
 * guess, bit for bit.  All frames of an iteration share one launch; a frame that has finished leaves it at once.  It has the
 * refusals and the context rule of viso_batch_fuse_tsdf.
 * An overflowed map refuses with VISO_ERR_NOMEM, as the getters do; a handle that is not a live TSDF map, or whose context is gone,
 * VISO_ERR_ARG.  The calls take the map's lock, like an extraction.
 * Limits: the gradient comes from 8 voxels, so the basin is about the gate wide; the distances are projective and averaged along the
 * fusing views' axes, so a surface at grazing incidence (80 degrees) pulls the pose off by tenths of a degree even from the truth;
 * below a voxel of about 0.05 m at KITTI's noise the steps stop shrinking before eps (status 2).  DESIGN.md 5.19 has the figures.
 * Out of scope: robust kernels beyond the gate, coarse-to-fine pyramids, alignment inside the KITTI runners, loop closure,
 * trilinear rendering.  Photometric terms from the gray sum: "TSDF photometric align" below.
 * HIP kernel (tsdf_align.hip): tsdf_linearize_kernel, the lanes of a wave consecutive pixels of a row, a thread strides over
 * several pixels.  Lanes whose k0 equals their left neighbour's form a run; the run's head lane alone does the eight probes and
 * loads, the others take the 8 x (weight, sum) from it.  The 28 sums stay in registers and are reduced once: across the wave by DPP,
 * across the workgroup's waves in LDS, then one set of 64-bit integer atomic adds per workgroup.  No float atomics, no scratch, no
 * workgroup waits for another. */
typedef struct viso_tsdf_align_params {   /* 48 bytes */
    uint32_t min_weight;     /* a voxel is usable from this many updates */
    double gate_voxels;      /* |distance| beyond this many voxels: the pixel is not used */
    int32_t max_iters;
    double eps_rot;          /* rad */
    double eps_trans;        /* m */
    int32_t min_pixels;      /* fewer used pixels: status -1 */
} viso_tsdf_align_params;

typedef struct viso_tsdf_normal {   /* 272 bytes */
    int64_t n[28];           /* step 9 */
    uint64_t n_points, n_used, n_missing, n_gated, n_clipped, n_out_of_range;
} viso_tsdf_normal;

typedef struct viso_tsdf_alignment {   /* 440 bytes */
    double pose[16];         /* the aligned pose, camera to world */
    double cov[36];          /* of (v, omega), row-major */
    double cost;             /* rms residual, pixels of disparity */
    uint64_t n_used;
    int32_t iters;           /* steps taken */
    int32_t status;          /* 1 converged, 2 max_iters reached, -1 too few pixels, -2 degenerate system, -3 a step that is not finite */
} viso_tsdf_alignment;

typedef struct viso_tsdf_align_step {   /* 400 bytes */
    double pose[16];         /* where the linearise was taken */
    viso_tsdf_normal normal;
} viso_tsdf_align_step;

/* min_weight 2, gate_voxels 1.0, max_iters 10, eps_rot 1e-6, eps_trans 1e-5, min_pixels 200.  Host only. */
void viso_tsdf_align_params_default(viso_tsdf_align_params* p);
/* Steps 1..9 at one pose.  Of *params, min_weight and gate_voxels are read (all of it is checked). */
int viso_tsdf_linearize(viso_tsdf* t, const viso_tsdf_align_params* params, const int16_t* disp, int rows, int cols, const viso_param* param,
                        const double* pose_or_null, viso_tsdf_normal* out);
int viso_tsdf_align(viso_tsdf* t, const viso_tsdf_align_params* params, const int16_t* disp, int rows, int cols, const viso_param* param,
                    const double* pose_guess_or_null, viso_tsdf_alignment* record_out, viso_tsdf_align_step* trace_out_or_null, int trace_cap);
/* poses_guess: [t1 - t0][16]; records_out: [t1 - t0]. */
int viso_batch_align_tsdf(viso_batch* b, viso_tsdf* t, int t0, int t1, const double* poses_guess, const viso_tsdf_align_params* params,
                          viso_tsdf_alignment* records_out);

/* ------------------------------------------------ TSDF photometric align: "TSDF align" with a second row a pixel, from the gray
 * sums (opt-in; NOT in the reference)
 *
 * A gray map ("TSDF intensity") keeps per voxel the sum of the intensities that updated it.  A used pixel of "TSDF align" therefore
 * also has a model intensity, sampled trilinearly from the same eight voxels, and the difference to the pixel's own intensity is a
 * second residual whose gradient comes from the model, not from the image: the pixel goes forward into the model.  The row holds the
 * motions inside a plane, which the signed distance leaves free (limit (iv) of DESIGN.md 5.19).  Its seven entries are rounded
 * to integers like the geometric ones and their products go into the same 28 sums, so the device output is bit-identical to
 * tests/photo_align_ref.py.  This definition is the contract.  Everything is IEEE double in the operand order written, with no
 * fused multiply-add.  The calls read the table only.  The calls of "TSDF align" are unchanged, on either kind of map.
 * Inputs of a linearise: those of viso_tsdf_linearize, and
 *   image        uint8 [rows][cols], the left image the map was computed from, pixel for pixel;
 *   photo_weight lambda, finite and >= 0: pixels of disparity per gray level, which puts the row into the units of the geometric
 *                one.  Default 1 / 32: a disparity residual is about 0.25 px, a voxel's mean intensity about 8 gray levels off on
 *                a ramp; the quotient, not tuned;
 *   photo_gate   finite and > 0, gray levels.  Default 255.0, which gates nothing.
 *   The map must be a gray map.  A plain map or a null image: VISO_ERR_ARG before a device is touched; the checks that do not need the
 *   map (those of "TSDF align", the image, lambda, the gate) come before the handle is looked at.  An overflowed map:
 *   VISO_ERR_NOMEM.
 * Per pixel (x, y): steps 1..8 of "TSDF align" are unchanged and decide whether the pixel is used; a used pixel's geometric row A is
 *   exactly the plain one and is added by step 9.  Then, for a used pixel:
 *   P1. i[dz][dy][dx] = (double)gray / (double)weight of the same eight voxels (usable by step 4: weight >= min_weight >= 1).
 *   P2. Step 5's interpolation on i with the same t, in the same operand order: mu for psi, E_0..2 for D_0..2.  h_i = E_i / voxel,
 *       gray levels per metre.
 *   P3. r = mu - (double)image[y][x].  |r| > photo_gate: n_photo_gated += 1, the pixel adds no photometric row (its geometric row
 *       stays).
 *   P4. hc_j = (T[0][j] h_0 + T[1][j] h_1) + T[2][j] h_2.  The row: b_0..2 = hc_j lambda;  b_3 = (Y hc_2 - Z hc_1) lambda,
 *       b_4 = (Z hc_0 - X hc_2) lambda,  b_5 = (X hc_1 - Y hc_0) lambda;  b_6 = r lambda.  There is no w: the residual is in
 *       measurement units already.
 *   P5. B_i = floor(b_i 256.0 + 0.5).  A value that is not finite or |B_i| >= 2^20: n_photo_clipped += 1, no photometric row.
 *   P6. n_photo_used += 1; for 0 <= i <= j <= 6: N[i][j] += B_i B_j, into the same 28 sums; p += B_6 B_6.
 *   Two products below 2^40 a pixel over at most 2^22 pixels: every sum stays below 2^63.  lambda = 0 gives B = 0: the 28 sums
 *   are those of viso_tsdf_linearize.
 * Output of a linearise: viso_tsdf_normal_gray; its `normal` holds the combined sums and the six counters of "TSDF align".
 * Align (viso_tsdf_align_gray): steps a..f of "TSDF align" on the combined N, min_pixels against n_used.  With C = N[6][6] / 65536.0
 *   and pp = p / 65536.0 of the final linearise:  a.cost = sqrt(C / n_used);  cost_geo = sqrt((C - pp) / n_used), pixels;
 *   cost_photo = sqrt(pp / n_photo_used) / lambda, gray levels, and 0 when lambda = 0 or n_photo_used = 0;
 *   a.cov = (C / max(n_used + n_photo_used - 6, 1)) H^-1.  On a status < 0, a.pose is the guess and every other number is zero.
 *   The trace's entries are viso_tsdf_align_gray_step, under the rules of viso_tsdf_align's.
 * Resident path: viso_batch_align_tsdf_gray is viso_batch_align_tsdf with frame t's image at images + (2 t) rows cols, the left
 *   images the run read; each record is what viso_tsdf_align_gray gives for that map, image and guess, bit for bit.
 *   VISO_ERR_ARG when the images' geometry is not the maps', as viso_batch_fuse_tsdf refuses on a gray map.
 * Limits: the texture must vary over several voxels (the model's intensity is a voxel mean; finer texture is averaged away and
 * aliases); constant exposure is assumed; the basin is still the gate's.  DESIGN.md 5.21 has the figures.
 * Out of scope: exposure or gain compensation, robust kernels beyond the gate, image pyramids, RGB.
 * HIP kernel (tsdf_align.hip): tsdf_gray_linearize_kernel, the body of tsdf_linearize_kernel instantiated with the intensity: a run's
 * head lane also loads the gray sums of its eight voxels and hands them to its run, the pixel's byte is read along the row, the
 * products of the second row add into the same 28 registers without a branch, and p and the three counters join the reduction:
 * 38 words a frame.  No float atomics, no scratch, no workgroup waits for another. */
typedef struct viso_tsdf_align_gray_params {   /* 64 bytes */
    viso_tsdf_align_params geo;
    double photo_weight;     /* lambda: pixels of disparity per gray level */
    double photo_gate;       /* gray levels */
} viso_tsdf_align_gray_params;

typedef struct viso_tsdf_normal_gray {   /* 304 bytes */
    viso_tsdf_normal normal; /* both rows' products; the counters of steps 1..9 */
    int64_t p;               /* the photometric part of N[6][6] */
    uint64_t n_photo_used, n_photo_gated, n_photo_clipped;
} viso_tsdf_normal_gray;

typedef struct viso_tsdf_alignment_gray {   /* 464 bytes */
    viso_tsdf_alignment a;
    double cost_geo;         /* rms geometric residual, pixels of disparity */
    double cost_photo;       /* rms photometric residual, gray levels */
    uint64_t n_photo_used;
} viso_tsdf_alignment_gray;

typedef struct viso_tsdf_align_gray_step {   /* 432 bytes */
    double pose[16];
    viso_tsdf_normal_gray normal;
} viso_tsdf_align_gray_step;

/* geo: viso_tsdf_align_params_default; photo_weight 1 / 32, photo_gate 255.0.  Host only. */
void viso_tsdf_align_gray_params_default(viso_tsdf_align_gray_params* p);
int viso_tsdf_linearize_gray(viso_tsdf* t, const viso_tsdf_align_gray_params* params, const int16_t* disp, const uint8_t* image, int rows,
                             int cols, const viso_param* param, const double* pose_or_null, viso_tsdf_normal_gray* out);
int viso_tsdf_align_gray(viso_tsdf* t, const viso_tsdf_align_gray_params* params, const int16_t* disp, const uint8_t* image, int rows, int cols,
                         const viso_param* param, const double* pose_guess_or_null, viso_tsdf_alignment_gray* record_out,
                         viso_tsdf_align_gray_step* trace_out_or_null, int trace_cap);
/* poses_guess: [t1 - t0][16]; records_out: [t1 - t0]. */
int viso_batch_align_tsdf_gray(viso_batch* b, viso_tsdf* t, int t0, int t1, const double* poses_guess,
                               const viso_tsdf_align_gray_params* params, viso_tsdf_alignment_gray* records_out);

/* ------------------------------------------------ Map eviction: the voxels outside a box leave a map, on the device (opt-in; NOT in
 * the reference)
 *
 * A voxel map or a TSDF map (plain or gray) lets go of every voxel outside an axis-aligned box of voxel indices and hands those
 * voxels back, so that a bounded table follows a camera over any distance.  The maps are integer and additive: the voxels evicted
 * along the way, merged by key with what is still in the table, are the map that was never evicted, bit for bit.
 *   What leaves: viso_*_evict removes every occupied voxel (count / weight >= 1) outside `keep` and nothing else; every surviving
 *     voxel keeps its count / weight, its sum(s) and its gray sum.
 *   What comes back: *n = the number removed; evicted_out receives them sorted by key, ascending, in the kind's own entry type,
 *     exactly as viso_*_get would have listed them before the call.  evicted_out == NULL discards them and ignores n_cap.  With a
 *     non-NULL output and n_cap < *n the call returns VISO_ERR_ARG with *n set, nothing written and nothing removed (the getters'
 *     rule).  viso_*_evict_count reads only.
 *   The box: voxel k is inside when lo[i] <= k[i] < hi[i] on every axis.  lo[i] > hi[i]: VISO_ERR_ARG.  lo[i] == hi[i] on any axis is
 *     an empty box: everything leaves and the table ends empty.  Values beyond +-2^20 are legal and contain everything on that side.
 *     viso_voxel_box_around (host only), per axis in IEEE double in this operand order: lo = (int64) floor((c - r) / voxel),
 *     hi = (int64) floor((c + r) / voxel) + 1, each clamped to int32; VISO_ERR_ARG for a centre, r or voxel that is not finite,
 *     r < 0, voxel not > 0, a null pointer.
 *   Kinds: viso_tsdf_evict on a gray map and viso_tsdf_evict_gray on a plain one return VISO_ERR_ARG; viso_tsdf_evict_count takes
 *     either kind.
 *   Counters: n_occupied falls by *n; every other counter is a history of what was fused and stays.
 *   Capacity comes back: after the call the table is as if the removed voxels had never been inserted: every survivor is found by
 *     the probes, no key is in the table twice, and every freed slot is an empty slot that the next insert can claim.  Nothing
 *     like a tombstone outlives the call.
 *   Refusals: an overflowed map refuses with VISO_ERR_NOMEM, like the getters; the handle rules of the maps apply; all argument
 *     checks (handle, kind, box, n) happen before a device is touched.
 *   Bounded loops: every loop on the device advances strictly and ends at the latest after one round of the slots (a bad table is
 *     a wrong answer, never a hang).
 * Device memory of a call: the list of the evicted voxels (none when they are discarded).  One exception: a table without a single
 * empty slot (exactly 2^capacity_log2 voxels, none dropped) is rebuilt through a list of its survivors.
 * Out of scope: growing or rehashing a table, un-overflowing a map, eviction by age or weight, eviction inside the batch's fuse
 * launches or the KITTI runners.
 * HIP kernels (voxel_hash.h, templates over the kind's payload, one thread per slot each): voxel_evict_mark_kernel counts, then lists
 * the voxels outside the box (one atomic per wave) and turns their keys into a reserved tombstone value; voxel_evict_rebuild_kernel
 * walks every probe cluster from its first slot and puts each live entry back at the first tombstone at or after its home slot;
 * voxel_evict_sweep_kernel turns the tombstones into empty slots and zeroes their payload.  The sort runs on the host. */
typedef struct viso_voxel_box { int32_t lo[3], hi[3]; } viso_voxel_box;   /* voxel k is inside when lo[i] <= k[i] < hi[i], i = 0, 1, 2 */

/* The box of the voxels that a cube of half-side half_side (metres) around centre touches.  Host only. */
int viso_voxel_box_around(const double centre[3], double half_side, double voxel, viso_voxel_box* out);
int viso_map_evict_count(viso_map* m, const viso_voxel_box* keep, size_t* n);
int viso_map_evict(viso_map* m, const viso_voxel_box* keep, viso_map_entry* evicted_out, size_t n_cap, size_t* n);
int viso_tsdf_evict_count(viso_tsdf* t, const viso_voxel_box* keep, size_t* n);
int viso_tsdf_evict(viso_tsdf* t, const viso_voxel_box* keep, viso_tsdf_entry* evicted_out, size_t n_cap, size_t* n);
int viso_tsdf_evict_gray(viso_tsdf* t, const viso_voxel_box* keep, viso_tsdf_gray_entry* evicted_out, size_t n_cap, size_t* n);

/* ------------------------------------------------ TSDF distance field: how far every voxel of a box is from the surface, on the
 * device (opt-in; NOT in the reference)
 *
 * For every voxel of an axis-aligned box of voxel indices, the squared distance in voxel units, an exact integer, to the nearest
 * surface voxel of the box: what a planner, a collision check or a clearance costmap asks of a map, without pulling the surface to
 * the host.  The call reads the table only (weight and sum: a plain and a gray map alike); the table, its statistics and the
 * overflow mark are untouched.  This definition is the contract; the device output is bit-identical to tests/field_ref.py.
 *   1. Box: n_i = hi[i] - lo[i], computed in int64, must be in 1..512 on every axis.  Cell (i0, i1, i2) is the voxel k = lo + i and
 *      is stored at index (i0 n1 + i1) n2 + i2 of sq_out and state_out.  n_cap counts cells: n_cap < n0 n1 n2 gives VISO_ERR_ARG
 *      and nothing is written.  The box may lie anywhere in int32.
 *   2. Usable voxel: every k_i in -2^20 .. 2^20 - 1, the voxel in the table, and its weight >= min_weight (min_weight >= 1, as for
 *      the getters).
 *   3. State, the low two bits: 0 unknown (not usable), 1 front (sum >= 0), 2 behind (sum < 0).
 *   4. Surface voxel: usable and, on some axis, with a usable neighbour k + e or k - e whose (sum < 0) differs: end a or end b of
 *      a crossing of rule 9 of "TSDF map" at the same min_weight.  The neighbour may lie outside the box.  A voxel at the first or
 *      the last index of an axis (k_i = -2^20, k_i = 2^20 - 1) has no neighbour on that side; nothing wraps.  A surface voxel's
 *      state also has VISO_FIELD_STATE_SURFACE set.
 *   5. Sites: the surface voxels inside the box; with VISO_FIELD_UNKNOWN_IS_SITE the unknown cells of the box too (the
 *      conservative field for planning: what was never seen counts as an obstacle).  Any other flag bit: VISO_ERR_ARG.  *n_sites
 *      is their number.
 *   6. Result: sq[c] = the minimum over the sites s of (c0 - s0)^2 + (c1 - s1)^2 + (c2 - s2)^2, at most 3 * 511^2;
 *      VISO_FIELD_NONE in every cell when the box holds no site.
 * Sites outside the box do not exist for the call: a value is exact only up to the cell's distance from the nearest face of the
 * box, so the caller pads the box by the clearance they care about.
 * An overflowed map refuses with VISO_ERR_NOMEM; a handle that is not a live TSDF map, or whose context is gone, VISO_ERR_ARG; no
 * device, VISO_ERR_HIP.  Every argument check (min_weight, box, flags, a null sq_out, n_cap, then the handle) happens before a
 * device is touched.  The call takes the map's lock, like an extraction.
 * Device memory of a call: two uint32 and one uint8 a cell (1.2 GB for the largest box); VISO_ERR_NOMEM when it cannot be
 * allocated.  Every loop on the device is bounded by an axis length (<= 512), by the at most 256 rounds of cells a block of the
 * first kernel takes, or is the probe's one round of the slots.
 * Out of scope: sites beyond the box and boxes longer than 512 voxels, sub-voxel distances, a field that stays on the device or is
 * updated as the map grows, fields of the voxel map, gradients of the field, anything in the batch runners.
 * HIP kernels (tsdf_field.hip), one thread per cell, the lanes of a wave adjacent along axis 2: tsdf_field_sites_kernel (the
 * cell's own read-only probe and at most six for its neighbours; the state, 0 at a site and VISO_FIELD_NONE elsewhere, the sites
 * counted with one ballot a round of 256 cells and one atomic per wave), then tsdf_field_pass_kernel three times, along axis 2, 1 and 0: the exact
 * Euclidean transform axis by axis, g'(i) = min_j g(j) + (i - j)^2 along a line, from one buffer into the other; the minimum is
 * searched outward from i and the search ends once d^2 >= the best value so far. */
#define VISO_FIELD_UNKNOWN_IS_SITE 1u
#define VISO_FIELD_STATE_SURFACE 4u
#define VISO_FIELD_NONE 0xffffffffu
/* sq_out: uint32 [n0][n1][n2]; state_out_or_null: uint8 of the same shape; n_sites_or_null: the number of sites. */
int viso_tsdf_distance_field(viso_tsdf* t, uint32_t min_weight, const viso_voxel_box* box, uint32_t flags,
                             uint32_t* sq_out, uint8_t* state_out_or_null, size_t n_cap, size_t* n_sites_or_null);

/* ------------------------------------------------ TSDF travel field: how far every voxel of a box is from a goal for a body that
 * keeps a clearance from the surface, on the device (opt-in; NOT in the reference)
 *
 * For every voxel of an axis-aligned box of voxel indices, the cost of the cheapest way to a goal through the cells that a sphere
 * of a given radius may occupy: whether a body gets from here to there, how far it is, and (following the costs downhill) which
 * way.  It is the geodesic question behind the distance field, and the first output of the map that depends on connectivity.  The
 * call reads the table only.  This definition is the contract; the device output is bit-identical to tests/travel_ref.py.
 *   1. Box, usable voxels, states, surface voxels, sites and sq: rules 1 to 6 of "TSDF distance field" with the same min_weight and
 *      flags; VISO_FIELD_UNKNOWN_IS_SITE is the only flag, any other bit VISO_ERR_ARG.  cost_out is stored like sq_out, and n_cap
 *      counts cells.  sq_out and state_out, where given, receive exactly what viso_tsdf_distance_field returns.
 *   2. Free cell: a cell of the box that is not behind the surface ((state & 3) != 2), is not a site, and has sq >= clearance_sq,
 *      VISO_FIELD_NONE counting as at least anything.  clearance_sq is any value below VISO_FIELD_NONE (0: no clearance);
 *      VISO_FIELD_NONE itself gives VISO_ERR_ARG.  Without the flag the unknown cells are free, the optimistic field; with it they
 *      are sites and never free, the conservative field.
 *   3. Goals: 1 <= n_goals <= 65536 absolute voxel indices [n_goals][3].  A goal outside the box, or whose cell is not free, is
 *      skipped; *n_goals_used is the number of entries of the list that were used (a cell named twice counts twice, and does no
 *      harm).  With no used goal every cell is VISO_FIELD_NONE and the call returns VISO_OK.
 *   4. Moves: from a free cell to any of its 26 neighbours inside the box that is free, at a cost of 3, 4 or 5 when 1, 2 or 3
 *      indices change: the <3,4,5> chamfer, in units of a third of a voxel.  There is no corner rule: a diagonal move is allowed
 *      whatever lies in the cells beside it.  Inflating the obstacles by the clearance is what keeps a path off the surface.
 *   5. Result: cost[c] = the smallest summed cost of a sequence of moves from c to a used goal: 0 at a used goal;
 *      VISO_FIELD_NONE where c is not free or no sequence exists; a finite value is at most 5 * 2^27.  *n_reached is the number
 *      of finite cells.  *n_rounds is the number of relaxation launches that found work: a diagnostic, not part of the bit-exact
 *      contract.
 *   6. Errors and locking follow the distance field.  Every argument check (min_weight, box, flags, clearance_sq, a null goals or
 *      cost_out, n_goals, n_cap, then the handle) happens before a device is touched, and a refused call writes nothing.  An
 *      overflowed map refuses with VISO_ERR_NOMEM; a handle that is not a live TSDF map, or whose context is gone, VISO_ERR_ARG.
 *      The call takes the map's lock and is a pure reader: the table, its statistics and the overflow mark are untouched.
 *   7. Bounds.  Device memory of a call: two uint32 and one uint8 a cell (the distance field's; the buffer its passes leave free
 *      holds the costs), three uint32 a tile of 8 x 8 x 8 cells, 12 bytes a goal and 8 words; VISO_ERR_NOMEM when it cannot be
 *      allocated.  Every loop on the device is bounded: the distance field's as stated there; a block of the cell kernels takes
 *      at most 256 rounds of cells; a tile is swept at most 513 times a visit (512 cells, and a chain of lowerings visits a cell
 *      once); a workgroup visits at most tiles / 2048 + 1 tiles a launch.  The host launches at most cells + 1 rounds: a cheapest
 *      sequence leaves a tile at a different cell every time, so it is settled after as many rounds as it has cells.  More
 *      returns VISO_ERR_HIP with a message; it is never a reason to go on.
 * In a box without obstacles the cost between two cells whose indices differ by (a >= b >= c >= 0), absolute values sorted, is
 * 3a + b + c.  So cost / 3 lies between 4 / (3 sqrt 2) = 0.943 and sqrt(11) / 3 = 1.106 times the Euclidean distance in voxels; the
 * extremes are along (1, 1, 0) and (3, 1, 1).
 * Out of scope: any-angle or smoothed paths; a field that stays on the device or is updated incrementally; bodies other than a
 * sphere; boxes over 512 voxels an axis; the voxel map; the batch runners.
 * HIP kernels (tsdf_travel.hip), behind the distance field's: tsdf_travel_init_kernel and tsdf_travel_goals_kernel (the starting
 * costs; a cell that is not free keeps a value of its own until the end), tsdf_travel_relax_kernel once a round (a workgroup per
 * listed tile: the tile and a halo of one cell in LDS, sweeps over the 26 neighbours until nothing falls, its own cells written
 * back, the neighbour tiles that see a lowered cell listed for the next round, each once), tsdf_travel_finish_kernel.  The launch
 * boundary is the only ordering between workgroups; the result is the unique fixed point whatever the schedule. */
/* goals: int32 [n_goals][3]; cost_out, sq_out_or_null: uint32 [n0][n1][n2]; state_out_or_null: uint8 of the same shape. */
int viso_tsdf_travel_field(viso_tsdf* t, uint32_t min_weight, const viso_voxel_box* box, uint32_t flags, uint32_t clearance_sq,
                           const int32_t* goals, size_t n_goals, uint32_t* cost_out, uint32_t* sq_out_or_null,
                           uint8_t* state_out_or_null, size_t n_cap, size_t* n_goals_used_or_null, size_t* n_reached_or_null,
                           size_t* n_rounds_or_null);

/* ------------------------------------------------ TSDF retract: fused frames taken out of the map again, so that poses can be
 * corrected (opt-in; NOT in the reference)
 *
 * A frame's pose is often known better after the frame has been fused: a window refinement, an alignment against the model, a loop
 * closure.  The weights, the sums and the gray sums of the table are integers, so fusing is adding, and an addition has an inverse:
 * subtracting the updates of a frame, computed from the same map, calibration, pose and fuse options, gives the table that never
 * saw the frame, bit for bit.  A move is that, followed by the fuse at the better pose.  This definition is the contract; the
 * device result is bit-identical to tests/retract_ref.py.
 *   1. Updates.  A retract of a frame (disp, rows, cols, param, pose, and image on a gray map) applies rules 1 to 6 of "TSDF map" to
 *      it, with the map's min_disp16 and its current fuse options (rules 3 and 7 of "TSDF fuse options"): exactly the updates
 *      (voxel, w, q, I) a fuse of the frame would make now.
 *   2. Take.  Rule 7 runs with the opposite sign, in the table's own arithmetic (weight modulo 2^32, sum and gray modulo 2^64):
 *      weight -= w, sum -= w q, gray -= w I.  Every update looks its voxel up read-only: no slot is claimed and no key written.
 *        An update whose voxel is not in the table changes nothing and counts in n_missing (updates, like n_dropped).
 *        A voxel whose weight the call takes below zero makes n_underflow non-zero: n_underflow != 0 exactly when at least one
 *        voxel underflows; its value is not part of the contract (which atomic sees the crossing depends on scheduling).
 *        The map's counters n_points, n_updates and n_out_of_range fall by what the same fuse would have added.
 *   3. Check, one read-only pass over the slots behind the take.
 *        n_freed: the voxels in the table with weight 0 whose sum, and gray on a gray map, are 0.
 *        n_inconsistent: the voxels with weight 0 and a sum or a gray that is not 0, and the voxels with weight > 0 and
 *        |sum| > T 1024 weight or gray > 255 weight: the bounds viso_tsdf_add_entries asks of an entry.
 *   4. Commit.  With n_missing, n_underflow and n_inconsistent all 0 the freed voxels leave the table as an eviction's do ("Map
 *      eviction", "Capacity comes back"): every survivor is found by the probes, every freed slot is an empty slot again, nothing
 *      like a tombstone outlives the call, and n_occupied falls by n_freed.  The call returns VISO_OK.  This is the eviction by
 *      weight that "Map eviction" leaves out, in its exact form: a voxel goes when its weight has returned to zero.
 *   5. Undo.  Otherwise the take runs again with the sign flipped.  It is find-only as well, so it touches exactly the same slots,
 *      and the modular additions restore every word, the three counters included: the map is bit for bit what it was.  The call
 *      returns VISO_ERR_ARG with an error text that names the three numbers.
 *   6. Report.  report (or NULL) receives six uint64 either way, in this order (VISO_RETRACT_*): n_points and n_updates of the
 *      retracted frames (what rule 2 took from the counters), n_missing, n_underflow, n_inconsistent, n_freed; the last two are the
 *      check's, taken behind the take and before any undo.  A call refused before the take writes nothing to it.
 *   7. Move: the retract at the old poses and, if it commits, the fuse at the new ones, under one hold on the map.  A refused
 *      retract fuses nothing and leaves the map unchanged.  A fuse that then fills the table returns VISO_ERR_NOMEM with the
 *      overflow mark, as any fuse does; the retract before it stays.
 *   8. Frames: the batch calls retract (move) the resident maps of frames t0 .. t1-1, a gray map's with the resident left images,
 *      in one call: one take, one check and one commit or undo for all of them, so the call stands or falls as a whole.
 * What the checks are: necessary conditions, not a proof that the frames were fused.  A frame that was never fused, but whose
 * updates all land on voxels of the table and leave every one of them within its bounds, passes, and leaves a valid table that
 * is the sum of no set of frames.  Retracting what was fused with other fuse options, another min_disp16, another calibration or
 * another pose is the caller's error; it is usually, but not always, refused.  The caller keeps its maps and poses (the batch
 * does); the map keeps no log of frames.
 * Eviction: voxels that were evicted since the fuse are missing, so the call is refused: retract before evicting, or retract from
 * a map rebuilt from the archive with viso_tsdf_add_entries (merge_entries in Python).
 * Refusals: the argument checks are those of the fuse calls, in the same order and with the same codes, before a device is
 * touched: the handle and its kind (viso_tsdf_retract on a gray map and the *_gray calls on a plain one: VISO_ERR_ARG), a non-null
 * map, calibration and (gray) image, sizes > 0, finite poses (a move: both) and calibration, then the context the batch and the map
 * must share.  An overflowed map refuses with VISO_ERR_NOMEM, like every other call (a map whose n_dropped is not 0 always carries
 * that mark).  A weight that wrapped beyond 2^32 while fusing is not detected.
 * Device memory of a call: none beyond the fuse's staging; a table without a single empty slot is rebuilt through a list of its
 * survivors, as in an eviction.  Every loop on the device is the fuse's march or a probe's one round of the slots.
 * Cost: the take is the fuse's march with read-only probes and the same atomics; a call adds the slot passes of a discarding
 * eviction (check, mark, rebuild, sweep) whatever the number of frames (DESIGN.md 5.26 has the measurements).
 * Out of scope: a retract for the voxel map; a list of the slots that reached zero, so that a small call skips the slot passes;
 * freeing deferred across calls; a log of fused frames inside the map; loop-closure detection and pose-graph optimisation.
 * HIP kernels: tsdf_take_kernel, tsdf_gray_take_kernel, tsdf_carve_take_kernel, tsdf_gray_carve_take_kernel (tsdf.hip): the four
 * fuse kernels' body with one more template flag, so the updates are the fuse's by construction: the loop over j uniform across
 * the wave, the runs of equal keys, the runs' sums by wave scans, and only a run's head lane at the table, where it finds (not
 * claims) the slot, adds the negated sums (the sums themselves in the undo: a runtime sign) and compares the weight its own atomic
 * returns with what it took; n_missing and the underflow flag by one atomic per wave and word, only when not zero.
 * voxel_retract_check_kernel and voxel_retract_mark_kernel (voxel_hash.h, templates over the kind's payload, one thread per
 * slot); the rebuild and the sweep are the eviction's kernels. */
#define VISO_RETRACT_N_POINTS 0
#define VISO_RETRACT_N_UPDATES 1
#define VISO_RETRACT_N_MISSING 2
#define VISO_RETRACT_N_UNDERFLOW 3
#define VISO_RETRACT_N_INCONSISTENT 4
#define VISO_RETRACT_N_FREED 5
int viso_tsdf_retract(viso_tsdf* t, const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_or_null,
                      uint64_t report_or_null[6]);
int viso_tsdf_retract_gray(viso_tsdf* t, const int16_t* disp, const uint8_t* image, int rows, int cols, const viso_param* param,
                           const double* pose_or_null, uint64_t report_or_null[6]);
/* poses [t1 - t0][16], as viso_batch_fuse_tsdf takes them and with its refusals */
int viso_batch_retract_tsdf(viso_batch* b, viso_tsdf* t, int t0, int t1, const double* poses, uint64_t report_or_null[6]);
int viso_tsdf_move(viso_tsdf* t, const int16_t* disp, int rows, int cols, const viso_param* param, const double* pose_old_or_null,
                   const double* pose_new_or_null, uint64_t report_or_null[6]);
int viso_tsdf_move_gray(viso_tsdf* t, const int16_t* disp, const uint8_t* image, int rows, int cols, const viso_param* param,
                        const double* pose_old_or_null, const double* pose_new_or_null, uint64_t report_or_null[6]);
int viso_batch_move_tsdf(viso_batch* b, viso_tsdf* t, int t0, int t1, const double* poses_old, const double* poses_new,
                         uint64_t report_or_null[6]);

/* ------------------------------------------------ pose graph: many relative poses and priors reconciled into one trajectory, on the
 * device (opt-in; NOT in the reference)
 *
 * The frame-to-frame motions with their covariances ("motion covariance"), the absolute poses of "TSDF align" and, later, loop
 * closures each say something about the trajectory; this is the step that makes one trajectory of them, which "TSDF retract"'s
 * move then applies to the map.  This definition is the contract; tests/posegraph_ref.py restates it in numpy.
 *   Nodes.  n_poses poses P_k, 4 x 4 row-major, camera to world: the matrices of chain_poses, viso_tsdf_fuse and viso_tsdf_align.
 *     The first three rows are read and taken as rigid.  fixed[k] != 0 (fixed_or_null NULL: none) keeps P_k as given, byte for byte.
 *   Edges.  n_edges edges (i, j, Z, Omega), edge_ij [n_edges][2], edge_Z [n_edges][16], edge_info [n_edges][36].  Z (first three
 *     rows read) measures P_i^-1 P_j.  i == -1 is a prior: P_-1 is the identity and never moves, so Z measures P_j itself.  j in
 *     0 .. n_poses-1, i in -1 .. n_poses-1, i != j; i > j is allowed, and several edges may join one pair.  Omega, 6 x 6 row-major
 *     (its lower triangle is read), is the symmetric positive definite information of the error in the tangent order (phi, rho),
 *     rotation first, of the right perturbation P = P^ Exp(xi) that viso_chain_covariances uses.  Its Cholesky factor C
 *     (Omega = C C') must pass the usual pivot test (> 1e-12 x the diagonal entry), else VISO_ERR_ARG.
 *   Cost.  r_e = Log(Z_e^-1 P_i^-1 P_j), F = 1/2 sum_e r_e' Omega_e r_e.
 *   Exp and Log.  xi = (phi, rho), theta = |phi|, K = [phi]x:  Exp(xi) = [R | V rho], R = I + a K + b K^2, V = I + b K + c1 K^2.
 *     Log(R, t): v = vee(R - R') / 2, theta = atan2(|v|, (trace R - 1) / 2), phi = v / a, rho = (I - K / 2 + cp K^2) t.
 *     a = sin(theta) / theta, b = (1 - cos(theta)) / theta^2, c1 = (theta - sin(theta)) / theta^3, cp = (1 - a / (2 b)) / theta^2, and for
 *     the Jacobians c2 = (theta^2 + 2 cos(theta) - 2) / (2 theta^4), c3 = (2 theta - 3 sin(theta) + theta cos(theta)) / (2 theta^5).
 *     For theta^2 < 1e-2 each is its series in x = theta^2, five terms: a = sum (-x)^k / (2k+1)!, b = sum (-x)^k / (2k+2)!,
 *     c1 = sum (-x)^k / (2k+3)!, c2 = sum (-x)^k / (2k+4)!, c3 = sum (k+1) (-x)^k / (2k+5)!,
 *     cp = 1/12 + x/720 + x^2/30240 + x^3/1209600 + x^4/47900160.  (The closed forms of c2, c3 and cp lose 1e-16 / theta^4 to
 *     cancellation, which is why the series start this early.)  A residual rotation near pi is outside the contract.
 *   Jacobians, exact (with J = I the iteration would stop where an approximate gradient vanishes, which is not the optimum):
 *     M = P_i^-1 P_j, J_j = J_r^-1(r), J_i = -J_r^-1(r) Ad(M^-1), Ad(T) = [[R, 0], [[t]x R, R]], and
 *     J_r^-1(xi) = [[A, 0], [-A Q A, A]], A = I - K/2 + cp K^2 at K = [-phi]x (the inverse of SO(3)'s left Jacobian at -phi), and
 *     Q = Q(-rho, -phi), Q(rho, phi) = G/2 + c1 (K G + G K + K G K) + c2 (K K G + G K K - 3 K G K) + c3 (K G K K + K K G K), G = [rho]x.
 *   Normal equations.  g_a = sum J_a' Omega r, H_ab = sum J_a' Omega J_b; fixed nodes and the world node have no columns.
 *   Step (Levenberg-Marquardt).  (H + lambda diag H) delta = -g.  lambda starts at 1e-4; an accepted trial multiplies it by 0.1, not
 *     below 1e-12; a rejected one by 10.
 *   One iteration.  Solve for delta.  max |delta| <= eps_step: status 1, the step is not applied.  Otherwise the trial is
 *     P_k <- P_k Exp(delta_k) for every k that is not fixed, with cost F'; it is accepted when F' <= F (1 + 2^-40) (the slack keeps
 *     rounding from rejecting the last steps).  Every solve counts as an iteration; max_iters solves without convergence give
 *     status 2, and the best poses are returned (fourth row 0 0 0 1; a fixed pose as given).
 *   Failures.  A pivot of the factorisations that is not > 1e-12 x its original diagonal entry: status -2.  A number that is not
 *     finite: status -3.  On a negative status poses_out equals poses, and the call still returns VISO_OK: the status is the report's.
 *   The solver is direct and uses the graph's shape.  An edge is a chain edge when i == -1 or |i - j| == 1, and long otherwise.
 *     The chain edges and the damping form a block-tridiagonal T; the L long edges are H_lambda = T + U U', where the 6 x 6 block of
 *     U for edge e at node a is J_a' C_e.  delta = y - W (I + U' W)^-1 U' y, y = T^-1 (-g), W = T^-1 U: one block-tridiagonal
 *     Cholesky, sweeps with 6 L + 1 right-hand sides and one dense Cholesky of order 6 L.
 *   Refusals (VISO_ERR_ARG, text in viso_last_error).  T must be definite on its own: the free nodes fall into runs joined by chain
 *     edges (a fixed node cuts a run), and every run needs a prior on one of its nodes or a chain edge to a fixed node; otherwise the
 *     call is refused and the text names the run's first node.  A free node with no edge at all is refused.  A caller whose
 *     odometry failed at a frame bridges the gap with a weak edge (a large covariance), or fixes a node on either side.  Poses, Z or
 *     Omega that are not finite are refused too.
 *   Limits.  n_poses 1 .. 65536, n_edges 1 .. 2^20, L <= 256, and the workspace -- 6 n_poses (6 L + 1) doubles, 158 a edge and the
 *     small blocks -- at most 2^28 doubles; beyond any of these VISO_ERR_UNSUPPORTED, before anything is allocated.
 *   Determinism.  Every sum has a fixed order: the edges of a node are added in edge-index order, reductions are fixed trees, and
 *     there is no float atomic.  Two calls with the same arrays give the same bytes.
 * viso_pose_graph_linearize: cost, gradient [n_poses][6] and, with step_out, the step [n_poses][6] of one solve at `lambda` (>= 0) at
 * the given poses; rows of fixed nodes are zeros.  A step whose factorisation fails is VISO_ERR_ARG.
 * viso_pose_graph_optimize: the loop.  max_iters 1 .. 200, eps_step >= 0.  report: VISO_PG_* below.  trace (or NULL with
 * trace_cap 0): one entry of five doubles a solve -- F, F' (F on the converged solve), lambda, max |delta|, accepted -- the first
 * trace_cap of them.
 * viso_motion_edge (host only): the edge of one solved frame, Z = inv(tr2mat(tr)) and info = (G cov G')^-1 with the G of
 * viso_chain_covariances, between the frame before (i) and the frame (j) of chain_poses' list; a cov whose G cov G' fails the pivot
 * test: VISO_ERR_ARG.
 * ctx_or_null: the context whose device and stream the call uses (NULL: the default context).  The checks that need no device come
 * first.  Device memory of a call: the one workspace block, allocated and freed by the call.
 * Out of scope: loop-closure detection; robust kernels on edges; marginal covariances of the optimised poses; graphs that are not a
 * chain plus at most 256 long edges; a factor of less serial depth (cyclic reduction, chain segments in parallel); the C++ host
 * mirror and the KITTI runners; the map's move inside the optimise call.
 * HIP kernels (posegraph.hip): pg_linearize_kernel (a thread an edge: r, the Jacobians, the edge's pieces J' C and C' r),
 * pg_assemble_kernel (a thread per node and entry, over the node's edge list), pg_cost_kernel, pg_chain_factor_kernel (a wave a run,
 * serial along it), pg_chain_solve_kernel (a lane a right-hand side), pg_capacitance_kernel, pg_dense_kernel (one workgroup),
 * pg_delta_kernel, pg_stepmax_kernel, pg_update_kernel. */
#define VISO_PG_STATUS 0
#define VISO_PG_ITERS 1
#define VISO_PG_COST_INITIAL 2
#define VISO_PG_COST_FINAL 3
#define VISO_PG_LAMBDA 4
#define VISO_PG_LAST_STEP 5
#define VISO_PG_N_LONG 6
#define VISO_PG_N_REJECTED 7
int viso_pose_graph_linearize(viso_ctx* ctx_or_null, int n_poses, const double* poses, const int32_t* fixed_or_null, int n_edges,
                              const int32_t* edge_ij, const double* edge_Z, const double* edge_info, double lambda, double* cost_out,
                              double* grad_out, double* step_out);
int viso_pose_graph_optimize(viso_ctx* ctx_or_null, int n_poses, const double* poses, const int32_t* fixed_or_null, int n_edges,
                             const int32_t* edge_ij, const double* edge_Z, const double* edge_info, int max_iters, double eps_step,
                             double* poses_out, double report[8], double* trace_or_null, int trace_cap);
int viso_motion_edge(const double tr[6], const double cov36[36], double Z[16], double info[36]);

/* ------------------------------------------------ loop closure: which earlier frames a frame looks like, and which of their features
 * are which of its own, on the device (opt-in; NOT in the reference)
 *
 * The producer of "pose graph"'s long edges.  A place signature per frame and an all-pairs search over the signatures of a sequence
 * name the candidate revisits; an ungated, mutual matcher over two frames' left-image descriptors gives the correspondences that the
 * existing solver (viso_ransac_minimize_reproj, viso_pose_covariance, viso_motion_edge) turns into an edge -- that glue is Python
 * (libviso_amd/loops.py).  No vocabulary, no training data, no images: the 121-element descriptors a batch already holds.  This
 * definition is the contract; tests/loop_ref.py restates it in numpy.
 *   Rows.  A descriptor row d[0..120] is taken as the integers of the matcher's packed rows: int16 values (direct calls), or the
 *     left-image rows of a batch's last run, whichever upload family filled them (the f32 and the int16 upload of the same integers
 *     give the same results).  Only the first n[f] rows of frame f are read.
 *   Word of a row.  For b = 0 .. bits-1: p_b = sum_k c[b][k] d[k], c[b][k] = +1 when bit (k mod 64) of draw (k div 64) is set and -1
 *     otherwise, the draws those of the viso_splitmix64 stream started at state seed * 0x9E3779B97F4A7C15 + b (mod 2^64).  Bit b of
 *     the word is p_b > 0.  Exact in int32 for |d| <= 1020 (any int16 row, in fact: 121 * 32768 < 2^31).
 *   Signature.  h[w] = min(number of the frame's rows with word w, 255), uint8 [1 << bits], bits in 6 .. 12; n = 0 gives zeros.
 *   Score.  s(j, i) = sum_w min(h_j[w], h_i[w]) (uint32), computed as (sum h_j + sum h_i - SAD(h_j, h_i)) / 2.
 *   Sequence sum.  S(j, i) = sum_{k = 0 .. seq_len-1, i - k >= 0} s(j - k, i - k), seq_len in 1 .. 16.
 *   Candidates of frame j.  The admissible i are 0 <= i <= j - min_gap (min_gap >= 1) with S(j, i) >= min_score.  They are picked
 *     greedily in the order (S descending, i ascending); a pick removes every i' with |i' - i| <= nms (nms >= 0); at most k (1 .. 16)
 *     are kept.  cand_out [n - j0][k] int32 (filled with -1) and score_out [n - j0][k] uint32 (filled with 0) hold rows j0 .. n-1.
 *   Wide match of a pair (query frame, target frame).  sad(q, t) = min(sum_k |Q_q[k] - T_t[k]|, 262142) (the bound is never met by
 *     rows within +-1020: 121 * 2040 = 246840).  For query q, t1 is the argmin over all targets by (sad, t) -- the LOWER index wins a
 *     tie, unlike viso_match_desc -- d1 its sad, d2 the least sad over t != t1 (+infinity with one target).  The row (q, t1, d1) is
 *     accepted when (double)d1 < (double)d2 * ratio and q is the argmin by (sad, q) over ALL queries for target t1.  match_out
 *     [np][cap][3] holds each pair's accepted rows in ascending q (zeros behind them), m_out [np] their counts.  Pairs may repeat,
 *     both frames of a pair may be the same, a frame without rows gives no match.
 * viso_place_signatures: desc [nf][cap][121] int16 (left images), n [nf] -> sig_out [nf][1 << bits].
 * viso_batch_place_signatures: the same for frames t0 .. t1-1 of the batch, from the resident rows; no descriptor leaves the device.
 * viso_place_scores: s_out [n - j0][n], row j - j0 holds s(j, i) for i <= j and 0 for i > j; a block above 2^31 bytes is refused with
 *   VISO_ERR_NOMEM.  viso_place_candidates: n <= 32768; the raw scores are held 16 MiB of rows at a time, so every n fits.
 * viso_wide_match: desc / n as above, pairs [np][2] of frame indices.  viso_batch_wide_match: frames of the batch.
 * Refusals (VISO_ERR_ARG with a text, before a device is touched): bits outside 6 .. 12, k or seq_len outside 1 .. 16, min_gap < 1,
 *   nms < 0, ratio outside (0, 1], n outside 1 .. 32768, cap outside 1 .. 16384, a count outside 0 .. cap, a null pointer, a pair that
 *   names a frame outside the range, a handle that is not live.  The batch calls need a batch of 121-element descriptors with a
 *   completed run (viso_batch_run*, matcher_only included) and say so otherwise; a frame whose f32 descriptors did not fit the packed
 *   rows (viso_batch_get_general_path_flags) is VISO_ERR_UNSUPPORTED.  A working block that does not fit the device: VISO_ERR_NOMEM.
 * ctx_or_null: the context whose device and stream a direct call uses (NULL: the default context); the calls are serialised with the
 *   other direct calls and use that context's scratch blocks (a named context needs no default one).  The batch calls read the rows AND
 *   the counts of the batch's last run: an upload or a detect since then changes nothing they see until the next run (the keypoints
 *   and counts the getters return are the upload's, so ask before uploading again).  They run on the batch's stream behind that run and use a
 *   workspace of the batch's own.
 * Determinism.  Counts, minima and maxima of integers only: no result depends on an order, two calls give the same bytes.
 * HIP kernels (loops.hip): loop_pack_kernel, place_sig_kernel, place_sums_kernel, place_score_kernel, place_cand_kernel,
 * wide_scan_kernel, wide_accept_kernel. */
int viso_place_signatures(viso_ctx* ctx_or_null, const int16_t* desc, const int32_t* n, int nf, int cap, uint64_t seed, int bits,
                          uint8_t* sig_out);
int viso_batch_place_signatures(viso_batch* b, int t0, int t1, uint64_t seed, int bits, uint8_t* sig_out);
int viso_place_scores(viso_ctx* ctx_or_null, const uint8_t* sig, int n, int bits, int j0, uint32_t* s_out);
int viso_place_candidates(viso_ctx* ctx_or_null, const uint8_t* sig, int n, int bits, int j0, int min_gap, int seq_len, int nms,
                          uint32_t min_score, int k, int32_t* cand_out, uint32_t* score_out);
int viso_wide_match(viso_ctx* ctx_or_null, const int16_t* desc, const int32_t* n, int nf, int cap, const int32_t* pairs, int np,
                    double ratio, int32_t* match_out, int32_t* m_out);
int viso_batch_wide_match(viso_batch* b, const int32_t* pairs, int np, double ratio, int32_t* match_out, int32_t* m_out);

#ifdef __cplusplus
}
#endif
#endif /* VISO_HIP_H_ */
