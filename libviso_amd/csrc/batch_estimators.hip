// batch_estimators.hip — the opt-in estimators behind a batch's RANSAC stage (none of them in the reference): motion covariance
// (covariance.hip), two-frame bundle adjustment (refine.hip), sliding-window bundle adjustment (window.hip).  Setters, the launches
// of a run, record getters.  The state is viso_batch::est (batch.h).
#include "batch.h"

// Opt-in motion covariance.  The records are allocated (zeroed) on the first request.
extern "C" int viso_batch_set_covariance(viso_batch* b, int mode, double sigma_px) {
    if (dead(b) || (mode != 0 && !motion_args_ok(mode, sigma_px))) {
        viso_set_error("viso_batch_set_covariance: bad argument (mode 0, 1, or 2 with a finite sigma_px > 0)");
        return VISO_ERR_ARG;
    }
    VISO_TRY(enter(b));
    if (mode && !b->est.cov.rec) {
        VISO_TRY(batch_sync(b));
        VISO_TRY(b->alloc_zeroed({{&b->est.cov.rec, (size_t)b->nf}}));
    }
    b->est.cov.mode = mode;
    b->est.cov.sigma = mode == 2 ? sigma_px : 0.0;
    return VISO_OK;
}

// Opt-in motion refinement.  The records and working buffers are allocated (zeroed) on the first request.
extern "C" int viso_batch_set_refine(viso_batch* b, int mode, double sigma_px) {
    if (dead(b) || (mode != 0 && !motion_args_ok(mode, sigma_px))) {
        viso_set_error("viso_batch_set_refine: bad argument (mode 0, 1, or 2 with a finite sigma_px > 0)");
        return VISO_ERR_ARG;
    }
    VISO_TRY(enter(b));
    BatchEstimators& E = b->est;
    if (mode && !E.ref.rec) {
        VISO_TRY(batch_sync(b));
        const size_t nf = (size_t)b->nf, c = (size_t)b->cap;
        VISO_TRY(b->alloc_zeroed({{&E.ref.rec, nf}, {&E.ref_pts, nf * 6 * c}, {&E.ref_idx, nf * c}}));
    }
    E.ref.mode = mode;
    E.ref.sigma = mode == 2 ? sigma_px : 0.0;
    return VISO_OK;
}

// Opt-in window refinement.  The records and working buffers are allocated (zeroed) on the first request with K > 0 and again for
// a larger K: the track and point buffers are sized (K - 1) cap per frame.
extern "C" int viso_batch_set_window_refine(viso_batch* b, int K, int mode, double sigma_px) {
    if (dead(b) || (K != 0 && !window_refine_args_ok(K, mode, sigma_px))) {
        viso_set_error("viso_batch_set_window_refine: bad argument (K 0, or K in 2..5 with mode 1, or mode 2 with a finite sigma_px > 0)");
        return VISO_ERR_ARG;
    }
    VISO_TRY(enter(b));
    BatchEstimators& E = b->est;
    if (K > E.win_kalloc) {
        VISO_TRY(batch_sync(b));
        E.win_kalloc = 0;
        const size_t nf = (size_t)b->nf, c = (size_t)b->cap, T = (size_t)(K - 1) * c;
        const std::initializer_list<DBuf> bufs = {{&E.win.rec, nf}, {&E.win_lp, nf * c}, {&E.win_nlp, nf}, {&E.win_tab, nf * 2 * c},
                                                  {&E.win_trk, nf * 5 * T}, {&E.win_pts, nf * 6 * T}};
        for (const DBuf& d : bufs) (void)b->release_bytes(d.p);   // those of a smaller K
        VISO_TRY(b->alloc_zeroed(bufs));
        E.win_kalloc = K;
    }
    E.win_K = K;
    E.win.mode = K ? mode : 0;
    E.win.sigma = K && mode == 2 ? sigma_px : 0.0;
    return VISO_OK;
}

// The estimators that are on, for frames 1 .. nf-1 (nf > 1), from what the refit left: tr, ok, the final inlier list.  None of them
// changes its inputs.
int batch_launch_estimators(viso_batch* b, hipStream_t ss) {
    const BatchEstimators& E = b->est;
    const size_t c = (size_t)b->cap;
    if (E.cov.mode) VISO_TRY(launch_motion_cov(ss, b->sitems, b->nf - 1, b->sp, E.cov.mode, E.cov.sigma, E.cov.rec + 1));
    if (E.ref.mode)
        VISO_TRY(launch_motion_refine(ss, b->sitems, b->nf - 1, b->sp, E.ref.mode, E.ref.sigma, E.ref_pts + 6 * c, E.ref_idx + c, c, E.ref.rec + 1));
    if (E.win_K) {   // over every frame's final inliers
        WinData d;
        d.X = b->Xp_c; d.obs = b->x_c; d.left = b->circ; d.left_fs = 4 * c; d.lstride = 4; d.lprev = 2;
        d.tr = b->tr; d.ok = b->ok; d.n_inl = b->n_inl; d.inl = b->inl; d.m = b->mc; d.ld = b->cap; d.tab = b->cap;
        WinWork w;
        w.Lp = E.win_lp; w.nLp = E.win_nlp; w.tabs = E.win_tab; w.maxT = (size_t)(E.win_K - 1) * c;
        w.trk = E.win_trk; w.pts = E.win_pts;
        VISO_TRY(launch_window_links(ss, d, w, 1, b->nf - 1));
        VISO_TRY(launch_window_refine(ss, d, w, b->sp, E.win_K, E.win.mode, E.win.sigma, 1, b->nf - 1, E.win.rec + 1));
    }
    return VISO_OK;
}

// An estimator's records of the last run (BatchRecords::last): after the batch's work in flight, an error naming `where` when that
// run computed none.
static int records_ready(viso_batch* b, int last, const char* where, const char* none) {
    VISO_TRY(batch_sync(b));
    if (!last) { viso_set_error("%s: the last run computed no %s", where, none); return VISO_ERR_ARG; }
    return VISO_OK;
}
#define COV_NONE "covariance (mode 0, or matcher_only)"
#define REF_NONE "refinement (mode 0, or matcher_only)"
#define WIN_NONE "window refinement (K = 0, or matcher_only)"

// The body of the record getters: frame t's record, or (all) the records of every frame, of the estimator whose state is member e.
template <class Rec>
static int get_records(viso_batch* b, bool all, int t, Rec* out, BatchRecords<Rec> BatchEstimators::*e, const char* where, const char* none) {
    if ((all ? dead(b) : !slot_ok(b, 0, t)) || !out) { viso_set_error("%s: bad argument", where); return VISO_ERR_ARG; }
    const BatchRecords<Rec>& R = b->est.*e;
    VISO_TRY(records_ready(b, R.last, where, none));
    HIP_TRY(hipMemcpy(out, R.rec + (all ? 0 : t), sizeof(Rec) * (all ? (size_t)b->nf : 1), hipMemcpyDeviceToHost));
    return VISO_OK;
}

extern "C" int viso_batch_get_covariance(viso_batch* b, int t, viso_motion_cov* out) {
    return get_records(b, false, t, out, &BatchEstimators::cov, "viso_batch_get_covariance", COV_NONE);
}
extern "C" int viso_batch_get_covariances(viso_batch* b, viso_motion_cov* out) {
    return get_records(b, true, 0, out, &BatchEstimators::cov, "viso_batch_get_covariances", COV_NONE);
}
extern "C" int viso_batch_get_refine(viso_batch* b, int t, viso_motion_refine* out) {
    return get_records(b, false, t, out, &BatchEstimators::ref, "viso_batch_get_refine", REF_NONE);
}
extern "C" int viso_batch_get_refines(viso_batch* b, viso_motion_refine* out) {
    return get_records(b, true, 0, out, &BatchEstimators::ref, "viso_batch_get_refines", REF_NONE);
}
extern "C" int viso_batch_get_window_refine(viso_batch* b, int t, viso_window_record* out) {
    return get_records(b, false, t, out, &BatchEstimators::win, "viso_batch_get_window_refine", WIN_NONE);
}
extern "C" int viso_batch_get_window_refines(viso_batch* b, viso_window_record* out) {
    return get_records(b, true, 0, out, &BatchEstimators::win, "viso_batch_get_window_refines", WIN_NONE);
}

// Frame t's refined points (the kernel leaves the final state in half 0 of the frame's point buffer) and L'.
extern "C" int viso_batch_get_refined_points(viso_batch* b, int t, int32_t* idx, double* X3xcap, int* n) {
    if (!slot_ok(b, 0, t) || !n) { viso_set_error("viso_batch_get_refined_points: bad argument"); return VISO_ERR_ARG; }
    const BatchEstimators& E = b->est;
    VISO_TRY(records_ready(b, E.ref.last, "viso_batch_get_refined_points", REF_NONE));
    viso_motion_refine rec;
    HIP_TRY(hipMemcpy(&rec, E.ref.rec + t, sizeof(rec), hipMemcpyDeviceToHost));
    const int nn = rec.status == 1 ? (rec.n < 0 ? 0 : rec.n > b->cap ? b->cap : rec.n) : 0;
    const size_t c = (size_t)b->cap;
    if (idx && nn) HIP_TRY(hipMemcpy(idx, E.ref_idx + (size_t)t * c, sizeof(int) * (size_t)nn, hipMemcpyDeviceToHost));
    if (X3xcap && nn)
        for (int row = 0; row < 3; ++row)
            HIP_TRY(hipMemcpy(X3xcap + (size_t)row * c, E.ref_pts + ((size_t)t * 6 + (size_t)row) * c, sizeof(double) * (size_t)nn, hipMemcpyDeviceToHost));
    *n = nn;
    return VISO_OK;
}
