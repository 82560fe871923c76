// batch_dense.hip — the dense side of a batch (none of it in the reference): disparity maps of every frame's resident pair by block
// matching (disparity.hip) or semi-global matching (sgm.hip), the speckle filter behind either (speckle.hip), and what consumes the
// maps: the getters, the reprojection to points, the fuse into a voxel map (voxelmap.hip).  The state is viso_batch::dense (batch.h).
#include "batch.h"

// Opt-in dense disparity (disparity.hip).  Only the parameters are kept here: the maps' buffer is allocated by the first launch
// that needs it.
extern "C" int viso_batch_set_disparity(viso_batch* b, const viso_disparity_params* params) {
    if (dead(b) || (params && !disparity_params_ok(params))) {
        viso_set_error("viso_batch_set_disparity: bad argument (NULL, or the parameters of include/viso_hip.h)");
        return VISO_ERR_ARG;
    }
    if (params && b->dense.sgm_on) {
        viso_set_error("viso_batch_set_disparity: semi-global matching is on (one method at a time: viso_batch_set_sgm(b, NULL) first)");
        return VISO_ERR_ARG;
    }
    VISO_TRY(enter(b));
    b->dense.disp_on = params != nullptr;
    if (params) b->dense.disp_p = *params;
    return VISO_OK;
}

// Opt-in semi-global matching (sgm.hip): the other method for the same maps.  Only the parameters are kept here: the workspace and
// the maps' buffer are allocated by the first launch that needs them.
extern "C" int viso_batch_set_sgm(viso_batch* b, const viso_sgm_params* params) {
    if (dead(b) || (params && !sgm_params_ok(params))) {
        viso_set_error("viso_batch_set_sgm: bad argument (NULL, or the parameters of include/viso_hip.h)");
        return VISO_ERR_ARG;
    }
    if (params && b->dense.disp_on) {
        viso_set_error("viso_batch_set_sgm: block matching is on (one method at a time: viso_batch_set_disparity(b, NULL) first)");
        return VISO_ERR_ARG;
    }
    VISO_TRY(enter(b));
    if (b->dense.sgm_on != (params != nullptr)) b->dense.last = 0;   // maps of the other state are not this one's
    b->dense.sgm_on = params != nullptr;
    if (params) b->dense.sgm_p = *params;
    return VISO_OK;
}

// Opt-in speckle filter of the maps (speckle.hip): a stage behind whichever method is on.  Only the parameters are kept here: the
// workspace is allocated by the first launch that needs it.  With no method on it does nothing.
extern "C" int viso_batch_set_speckle(viso_batch* b, const viso_speckle_params* params) {
    if (dead(b) || (params && !speckle_params_ok(params))) {
        viso_set_error("viso_batch_set_speckle: bad argument (NULL, or the parameters of include/viso_hip.h)");
        return VISO_ERR_ARG;
    }
    VISO_TRY(enter(b));
    BatchDense& D = b->dense;
    const bool same = D.spk_on == (params != nullptr) && (!params || (D.spk_p.max_size == params->max_size && D.spk_p.max_diff == params->max_diff));
    if (!same) D.last = 0;   // maps of the other state are not this one's
    D.spk_on = params != nullptr;
    if (params) D.spk_p = *params;
    return VISO_OK;
}

// What a dense launch over the batch's resident images cannot do, found before anything of the run is issued: images wider than
// the kernels handle, and workspaces of which not even one frame's fits the caps.
int dense_preflight(viso_batch* b, const char* where) {
    const BatchDense& D = b->dense;
    if (!disparity_geometry_ok(b->img_rows, b->img_cols)) {
        viso_set_error("%s: dense disparity of %d-column images is beyond this build (2048 at most)", where, b->img_cols);
        return VISO_ERR_UNSUPPORTED;
    }
    if (D.sgm_on) VISO_TRY(sgm_group_frames(where, b->img_rows, b->img_cols, D.sgm_p.num_disp, b->nf, nullptr));
    if (D.speckle() && !speckle_geometry_ok(b->img_rows, b->img_cols)) {
        viso_set_error("%s: the speckle filter of %d x %d maps is beyond this build (2^31 - 1 pixels)", where, b->img_rows, b->img_cols);
        return VISO_ERR_UNSUPPORTED;
    }
    if (D.speckle()) VISO_TRY(speckle_group_frames(where, b->img_rows, b->img_cols, b->nf, nullptr));
    return VISO_OK;
}

// The speckle filter over the batch's maps, in place, behind the method's launches on the context's stream (viso_batch_set_speckle
// on with max_size > 0), group by group through the batch's workspace.
static int launch_batch_speckle(viso_batch* b, const char* where) {
    BatchDense& D = b->dense;
    int group;
    VISO_TRY(speckle_group_frames(where, b->img_rows, b->img_cols, b->nf, &group));   // fails when the cap moved since dense_preflight
    VISO_TRY(b->fit(&D.spk_ws, &D.spk_ws_bytes, speckle_frame_bytes(b->img_rows, b->img_cols) * (size_t)group, false, where,
                    "speckle workspace (viso_speckle_set_workspace_cap)"));
    return launch_speckle(b->ctx->stream, D.disp, (size_t)b->img_rows * b->img_cols, b->img_rows, b->img_cols, b->nf, &D.spk_p, D.spk_ws, group);
}

// The disparity of every frame's resident pair on the context's stream (a method on, images present, dense_preflight passed, the
// device entered by the caller).  The maps' buffer follows the image geometry: (re)allocated here, after the batch's work in flight.
int launch_batch_disparity(viso_batch* b, const char* where) {
    BatchDense& D = b->dense;
    const size_t per = (size_t)b->img_rows * b->img_cols;
    D.last = 0;
    VISO_TRY(b->fit(&D.disp, &D.disp_bytes, sizeof(int16_t) * per * (size_t)b->nf));
    D.rows = b->img_rows; D.cols = b->img_cols;
    if (D.sgm_on) {   // the same maps by semi-global matching, group by group through the batch's workspace
        int group;
        VISO_TRY(sgm_group_frames(where, b->img_rows, b->img_cols, D.sgm_p.num_disp, b->nf, &group));   // fails when the cap moved since dense_preflight
        VISO_TRY(b->fit(&D.sgm_ws, &D.sgm_ws_bytes, sgm_frame_bytes(b->img_rows, b->img_cols, D.sgm_p.num_disp) * (size_t)group, false, where,
                        "SGM workspace (viso_sgm_set_workspace_cap)"));
        VISO_TRY(launch_sgm(b->ctx->stream, batch_images(b, 0, b->nf), &D.sgm_p, D.disp, per, D.sgm_ws, group));
    } else {
        VISO_TRY(launch_disparity(b->ctx->stream, batch_images(b, 0, b->nf), &D.disp_p, D.disp, per));
    }
    if (D.speckle()) VISO_TRY(launch_batch_speckle(b, where));
    D.last = 1;
    return VISO_OK;
}

// Only the disparity, over images uploaded without keypoints.
extern "C" int viso_batch_run_disparity(viso_batch* b) {
    const char* where = "viso_batch_run_disparity";
    if (dead(b) || !b->dense.on() || !b->images) { viso_set_error("%s: dense disparity is off, or no images are uploaded", where); return VISO_ERR_ARG; }
    VISO_TRY(dense_preflight(b, where));
    VISO_TRY(enter(b));
    return launch_batch_disparity(b, where);
}

// The maps' consumers: refused while no method is on, or no run has computed maps of the present state.
static int dense_ready(const viso_batch* b, const char* where) {
    if (b->dense.on() && b->dense.last) return VISO_OK;
    viso_set_error("%s: dense disparity is off, or no run has computed it", where);
    return VISO_ERR_ARG;
}

static int get_disparity(viso_batch* b, bool all, int t, int16_t* out, const char* where) {
    if (dead(b) || (!all && (t < 0 || t >= b->nf)) || !out) { viso_set_error("%s: bad argument", where); return VISO_ERR_ARG; }
    VISO_TRY(dense_ready(b, where));
    VISO_TRY(enter(b));
    VISO_TRY(batch_sync(b));
    const size_t per = (size_t)b->dense.rows * b->dense.cols;
    HIP_TRY(hipMemcpy(out, b->dense.disp + (all ? 0 : (size_t)t * per), sizeof(int16_t) * per * (all ? (size_t)b->nf : 1), hipMemcpyDeviceToHost));
    return VISO_OK;
}

extern "C" int viso_batch_get_disparity(viso_batch* b, int t, int16_t* out) { return get_disparity(b, false, t, out, "viso_batch_get_disparity"); }

extern "C" int viso_batch_get_disparities(viso_batch* b, int16_t* out) { return get_disparity(b, true, 0, out, "viso_batch_get_disparities"); }

// The resident maps of frames t0 .. t1-1 as a view (common.h) with the batch's calibration, at `poses` [t1 - t0][16] (or null).
// needs (or null): who needs the resident left images the maps were computed from (batch_images); the view then has
// them, and they must still be there with the maps' geometry.  The one place that knows where a frame's map lies.
static int dense_view(const char* where, const viso_batch* b, int t0, int t1, const double* poses, const char* needs, DispView* v) {
    const BatchDense& D = b->dense;
    const size_t per = (size_t)D.rows * D.cols;
    if (needs && (!b->images || b->img_rows != D.rows || b->img_cols != D.cols)) {
        viso_set_error("%s: the resident images (%d x %d) are not the maps' (%d x %d): %s needs the images the maps were computed from",
                       where, b->images ? b->img_cols : 0, b->images ? b->img_rows : 0, D.cols, D.rows, needs);
        return VISO_ERR_ARG;
    }
    const StereoImages im = needs ? batch_images(b, t0, t1 - t0) : StereoImages{};   // each frame's left image; none: null and a stride of 0
    *v = DispView{D.disp + (size_t)t0 * per, per, im.img, im.fs, D.rows, D.cols, t1 - t0,
                  StereoCalib{b->sp.f, b->sp.cu, b->sp.cv, b->sp.base}, poses, b->ctx};
    return VISO_OK;
}

// Frame t's resident map as an organised point image [rows][cols][3] f32 (speckle.hip), computed on demand with the batch's
// calibration; the batch keeps no point buffer (the call's own is freed before it returns, so it is not recorded as the batch's).
extern "C" int viso_batch_get_disparity_points(viso_batch* b, int t, const double* pose_or_null, int min_disp16, float* out) {
    const char* where = "viso_batch_get_disparity_points";
    if (dead(b) || t < 0 || t >= b->nf || !out || min_disp16 < 1) { viso_set_error("%s: bad argument", where); return VISO_ERR_ARG; }
    if (!b->params_set) { viso_set_error("%s: parameters not set (the calibration comes from viso_batch_set_params)", where); return VISO_ERR_ARG; }
    VISO_TRY(dense_ready(b, where));
    VISO_TRY(enter(b));
    DispView v;
    VISO_TRY(dense_view(where, b, t, t + 1, pose_or_null, nullptr, &v));
    const size_t per = v.px();
    float* dout = nullptr;
    if (hipMalloc((void**)&dout, 3 * sizeof(float) * per) != hipSuccess) {
        (void)hipGetLastError();
        viso_set_error("%s: cannot allocate the %zu-byte point image", where, 3 * sizeof(float) * per);
        return VISO_ERR_NOMEM;
    }
    hipStream_t s = b->ctx->stream;
    const int r = launch_points(s, v, min_disp16, dout);
    hipError_t e = hipSuccess;
    if (r >= 0) e = hipMemcpyAsync(out, dout, 3 * sizeof(float) * per, hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    (void)hipFree(dout);
    VISO_TRY(r);
    HIP_TRY(e);
    HIP_TRY(e2);
    return VISO_OK;
}

// What viso_batch_fuse_disparities and viso_batch_fuse_tsdf check before they hand over (`map`: the handle, only compared with null).
static int fuse_prelude(const char* where, viso_batch* b, const void* map, int t0, int t1, const double* poses) {
    if (dead(b) || !map || t0 < 0 || t1 > b->nf || t0 >= t1 || !poses) {
        viso_set_error("%s: bad argument (live handles, 0 <= t0 < t1 <= n_frames, poses [t1 - t0][16])", where);
        return VISO_ERR_ARG;
    }
    if (!b->params_set) { viso_set_error("%s: parameters not set (the calibration comes from viso_batch_set_params)", where); return VISO_ERR_ARG; }
    VISO_TRY(dense_ready(b, where));
    return enter(b);
}

// The resident maps of frames t0 .. t1-1 into a voxel map of the same context (voxelmap.hip), with the batch's calibration: on the
// context's stream, behind the run that computed them, with no host copy of the maps.
extern "C" int viso_batch_fuse_disparities(viso_batch* b, viso_map* m, int t0, int t1, const double* poses) {
    const char* where = "viso_batch_fuse_disparities";
    VISO_TRY(fuse_prelude(where, b, m, t0, t1, poses));
    DispView v;
    VISO_TRY(dense_view(where, b, t0, t1, poses, nullptr, &v));
    return map_fuse_resident(where, m, v);
}

// The same into a TSDF map of the same context (tsdf.hip).  A gray map also reads the resident left images the maps were computed
// from (frame t's at images + 2 t per): they must still be there, with the maps' geometry.
extern "C" int viso_batch_fuse_tsdf(viso_batch* b, viso_tsdf* t, int t0, int t1, const double* poses) {
    const char* where = "viso_batch_fuse_tsdf";
    VISO_TRY(fuse_prelude(where, b, t, t0, t1, poses));
    DispView v;
    VISO_TRY(dense_view(where, b, t0, t1, poses, tsdf_is_gray(t) ? "a gray TSDF map" : nullptr, &v));
    return tsdf_fuse_resident(where, t, v);
}

// The resident maps of frames t0 .. t1-1 taken out of a TSDF map again (tsdf.hip; include/viso_hip.h, "TSDF retract"), at the poses
// they were fused at; a gray map's with the resident left images, as the fuse.  One take, one check and one commit or undo for all.
extern "C" int viso_batch_retract_tsdf(viso_batch* b, viso_tsdf* t, int t0, int t1, const double* poses, uint64_t report_or_null[6]) {
    const char* where = "viso_batch_retract_tsdf";
    VISO_TRY(fuse_prelude(where, b, t, t0, t1, poses));
    DispView v;
    VISO_TRY(dense_view(where, b, t0, t1, poses, tsdf_is_gray(t) ? "a gray TSDF map" : nullptr, &v));
    return tsdf_retract_resident(where, t, v, false, nullptr, report_or_null);
}

// The same, and the frames fused again at poses_new behind it, under one hold on the map: a refused retract fuses nothing.
extern "C" int viso_batch_move_tsdf(viso_batch* b, viso_tsdf* t, int t0, int t1, const double* poses_old, const double* poses_new,
                                    uint64_t report_or_null[6]) {
    const char* where = "viso_batch_move_tsdf";
    if (!poses_new) { viso_set_error("%s: bad argument (poses_new [t1 - t0][16])", where); return VISO_ERR_ARG; }
    VISO_TRY(fuse_prelude(where, b, t, t0, t1, poses_old));
    DispView v;
    VISO_TRY(dense_view(where, b, t0, t1, poses_old, tsdf_is_gray(t) ? "a gray TSDF map" : nullptr, &v));
    return tsdf_retract_resident(where, t, v, true, poses_new, report_or_null);
}

// The resident maps of frames t0 .. t1-1 aligned against a TSDF map of the same context (tsdf_align.hip), each on its own from its
// guess, with the batch's calibration and no host copy of the maps.  The refusals of viso_batch_fuse_tsdf.
extern "C" int viso_batch_align_tsdf(viso_batch* b, viso_tsdf* t, int t0, int t1, const double* poses_guess, const viso_tsdf_align_params* params,
                                     viso_tsdf_alignment* records_out) {
    const char* where = "viso_batch_align_tsdf";
    if (!params || !records_out) { viso_set_error("%s: bad argument (non-null parameters and records)", where); return VISO_ERR_ARG; }
    VISO_TRY(fuse_prelude(where, b, t, t0, t1, poses_guess));
    DispView v;
    VISO_TRY(dense_view(where, b, t0, t1, poses_guess, nullptr, &v));
    return tsdf_align_resident(where, t, v, params, records_out);
}

// The same with the photometric row (tsdf_align.hip, "TSDF photometric align"): frame t's left image at images + 2 t per, which must
// still be there with the maps' geometry, as viso_batch_fuse_tsdf asks of them for a gray map.
extern "C" int viso_batch_align_tsdf_gray(viso_batch* b, viso_tsdf* t, int t0, int t1, const double* poses_guess,
                                          const viso_tsdf_align_gray_params* params, viso_tsdf_alignment_gray* records_out) {
    const char* where = "viso_batch_align_tsdf_gray";
    if (!params || !records_out) { viso_set_error("%s: bad argument (non-null parameters and records)", where); return VISO_ERR_ARG; }
    VISO_TRY(fuse_prelude(where, b, t, t0, t1, poses_guess));
    DispView v;
    VISO_TRY(dense_view(where, b, t0, t1, poses_guess, "the photometric row", &v));
    return tsdf_align_gray_resident(where, t, v, params, records_out);
}
