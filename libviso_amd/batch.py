"""The batched, device-resident family of include/viso_hip.h (csrc/batch.hip): a Context, the Batch of stereo frames resident in
HBM with its uploads, runs, opt-in stages and getters, and pinned host memory for the asynchronous uploads."""
import ctypes as C
import weakref

import numpy as np

from . import VisoError, _call, _f32, _Handle, _i32, _pose_arg, _sigma, _struct_arg, load
from .abi import (DESC_LEN, MOTION_COV_DTYPE, MOTION_REFINE_DTYPE, TSDF_ALIGNMENT_DTYPE, TSDF_ALIGNMENT_GRAY_DTYPE, WINDOW_RECORD_DTYPE,
                  DisparityParams, SgmParams, SpeckleParams, ptr)
from .dense import _map_pair, disparity_params, sgm_params, speckle_params
from .maps import _reported, tsdf_align_gray_params, tsdf_align_params
from .plain import HARRIS_K


def _created(L, where, h):
    """The handle a constructor of the library returned, or its failure."""
    if not h:
        raise VisoError(where + ": " + L.viso_last_error().decode())
    return h


class PinnedArray(_Handle):
    """numpy view of hipHostMalloc memory (viso_host_alloc) for the *_async uploads."""
    _destroy = "viso_host_free"

    def __init__(self, shape, dtype):
        self.L = load()
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._own(_created(self.L, "viso_host_alloc", self.L.viso_host_alloc(self.nbytes)))
        buf = (C.c_char * self.nbytes).from_address(self.h)
        self.a = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def close(self):
        self.a = None
        super().close()


class Context(_Handle):
    _destroy, _close_last = "viso_ctx_destroy", True

    def __init__(self, device=0, stream=None):
        self.L = load()
        self._batches = weakref.WeakSet()   # closed with the context: a batch destroyed after its context uses freed streams
        self._own(_created(self.L, "viso_ctx_create", self.L.viso_ctx_create(device, stream)))

    def synchronize(self):
        _call(self.L.viso_ctx_synchronize, self.h)

    def close(self):
        if self.h:
            # its batches first, whatever order the caller (or the garbage collector, after an exception skipped the
            # caller's close() calls) takes: viso_batch_destroy on a destroyed context aborts inside the HIP runtime
            for b in list(self._batches):
                try:
                    b.close()
                except Exception:
                    pass
        super().close()


class Batch(_Handle):
    """viso_batch: n_frames stereo frames resident in HBM (include/viso_hip.h)."""
    _destroy = "viso_batch_destroy"

    def __init__(self, ctx, n_frames, cap, dlen=DESC_LEN):
        self.ctx, self.L = ctx, ctx.L
        self.nf, self.cap, self.dlen = n_frames, cap, dlen
        self._own(_created(self.L, "viso_batch_create", self.L.viso_batch_create(ctx.h, n_frames, cap, dlen)))
        ctx._batches.add(self)

    def upload(self, kp, desc, n, f0=0):
        kp, desc, n = _f32(kp), _f32(desc), _i32(n)
        nf = kp.shape[0]
        assert kp.shape == (nf, 2, self.cap, 2) and desc.shape == (nf, 2, self.cap, self.dlen)
        _call(self.L.viso_batch_upload, self.h, f0, nf, ptr(kp, C.c_float), ptr(desc, C.c_float), ptr(n, C.c_int32))

    def upload_async(self, kp, desc, n, f0=0):
        """Enqueue the copies on the context's stream; kp/desc should be PinnedArray views and must stay untouched
        until the stream has passed them."""
        assert kp.dtype == np.float32 and desc.dtype == np.float32 and kp.flags.c_contiguous and desc.flags.c_contiguous
        n = _i32(n)
        nf = kp.shape[0]
        _call(self.L.viso_batch_upload_async, self.h, f0, nf, ptr(kp, C.c_float), ptr(desc, C.c_float), ptr(n, C.c_int32))

    def upload_i16(self, kp, desc16, n, f0=0, asynchronous=False):
        """Descriptors as int16 [nf][2][cap][dlen] (the lossless encoding of the Sobel windows; half the bytes).
        asynchronous=True: enqueued on the context's stream; kp / desc16 should be PinnedArray views."""
        kp, n = _f32(kp), _i32(n)
        assert desc16.dtype == np.int16 and desc16.flags.c_contiguous
        nf = kp.shape[0]
        assert kp.shape == (nf, 2, self.cap, 2) and desc16.shape == (nf, 2, self.cap, self.dlen)
        fn = self.L.viso_batch_upload_i16_async if asynchronous else self.L.viso_batch_upload_i16
        _call(fn, self.h, f0, nf, ptr(kp, C.c_float), ptr(desc16, C.c_int16), ptr(n, C.c_int32))

    def upload_images_async(self, images, kp, n, f0=0):
        assert images.dtype == np.uint8 and images.flags.c_contiguous and kp.dtype == np.float32 and kp.flags.c_contiguous
        n = _i32(n)
        nf, _, rows, cols = images.shape
        _call(self.L.viso_batch_upload_images_async, self.h, f0, nf, ptr(images, C.c_uint8), rows, cols, ptr(kp, C.c_float),
              ptr(n, C.c_int32))

    def upload_images(self, images, kp, n, f0=0):
        """Image-in mode: uint8 images [nf][2][rows][cols] + keypoints (descriptors are extracted on the device)."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        kp, n = _f32(kp), _i32(n)
        nf, _, rows, cols = images.shape
        assert kp.shape == (nf, 2, self.cap, 2)
        _call(self.L.viso_batch_upload_images, self.h, f0, nf, ptr(images, C.c_uint8), rows, cols, ptr(kp, C.c_float), ptr(n, C.c_int32))

    def upload_images_only(self, images, f0=0):
        """Images without keypoints: follow with detect()."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        nf, _, rows, cols = images.shape
        _call(self.L.viso_batch_upload_images, self.h, f0, nf, ptr(images, C.c_uint8), rows, cols, None, None)

    def detect(self, n_features=1200, nbinx=24, nbiny=5, k=HARRIS_K):
        _call(self.L.viso_batch_detect, self.h, n_features, nbinx, nbiny, k)

    def keypoints(self, t, side):
        kp = np.empty((self.cap, 2), np.float32)
        n = C.c_int(0)
        _call(self.L.viso_batch_get_keypoints, self.h, t, side, ptr(kp, C.c_float), C.byref(n))
        return kp[:n.value].copy()

    def run_images(self, matcher_only=False):
        _call(self.L.viso_batch_run_images, self.h, int(matcher_only))

    def set_subpixel(self, mode):
        """viso_batch_set_subpixel: 0 = off (default), 1 = refine the stereo matches' uR, 2 = uR and vR (image-in runs only)."""
        _call(self.L.viso_batch_set_subpixel, self.h, int(mode))

    def subpixel(self, t):
        """(n, 2) float32 refined (uR', vR') of frame t's stereo rows from the last run, in the order of matches(0, t)."""
        out = np.empty((self.cap, 2), np.float32)
        n = C.c_int(0)
        _call(self.L.viso_batch_get_subpixel, self.h, t, ptr(out, C.c_float), C.byref(n))
        return out[:n.value].copy()

    def set_rectify(self, raw_shape, out_shape=None, left=None, right=None, border=0):
        """viso_batch_set_rectify: from the next image upload on, uploads take raw images of raw_shape (rows, cols) and the device
        rectifies them to out_shape with the maps left = (mapx, mapy) and right = (mapx, mapy) (rectify_map).  set_rectify(None)
        turns it off."""
        if raw_shape is None:
            _call(self.L.viso_batch_set_rectify, self.h, 0, 0, 0, 0, None, None, None, None, 0)
            return
        if left is None or right is None or out_shape is None:
            raise ValueError("set_rectify: out_shape and both maps are needed (or raw_shape=None to turn it off)")
        rows, cols = (int(v) for v in out_shape)
        lx, ly = _map_pair(left[0], left[1], (rows, cols))
        rx, ry = _map_pair(right[0], right[1], (rows, cols))
        rr, rc = (int(v) for v in raw_shape)
        _call(self.L.viso_batch_set_rectify, self.h, rr, rc, rows, cols, ptr(lx, C.c_float), ptr(ly, C.c_float), ptr(rx, C.c_float),
              ptr(ry, C.c_float), int(border))

    def image_shape(self):
        """(rows, cols) of the device images (viso_batch_get_image_geometry); (0, 0) before any image upload."""
        r, c = C.c_int(0), C.c_int(0)
        _call(self.L.viso_batch_get_image_geometry, self.h, C.byref(r), C.byref(c))
        return r.value, c.value

    def image(self, t, side):
        """The device image of frame t, side (uint8, rectified when rectification was on at its upload)."""
        shape = self.image_shape()   # the library's geometry, not a copy of it here: the buffer always fits what is copied
        if shape == (0, 0):
            raise VisoError("Batch.image: no images uploaded")
        out = np.empty(shape, np.uint8)
        _call(self.L.viso_batch_get_image, self.h, int(t), int(side), ptr(out, C.c_uint8))
        return out

    def _set_dense(self, fn, Struct, make, params, kw, a="a"):
        """viso_batch_set_<stage>(params): None and no keywords turn the stage off, anything else is what _struct_arg takes."""
        if params is None and not kw:
            _call(fn, self.h, None)
        else:
            _call(fn, self.h, C.byref(_struct_arg(fn.__name__[len("viso_batch_"):], Struct, make, params, kw, a)))

    def set_disparity(self, params=None, **kw):
        """viso_batch_set_disparity: dense disparity of every frame's resident pair in the next image-in runs (run_images, also
        matcher_only) and in run_disparity.  params: a DisparityParams, a dict of its fields, or keyword fields (defaults for the
        rest); set_disparity(None) turns it off (the default)."""
        self._set_dense(self.L.viso_batch_set_disparity, DisparityParams, disparity_params, params, kw)

    def set_sgm(self, params=None, **kw):
        """viso_batch_set_sgm: the batch's dense maps by semi-global matching in the next image-in runs and in run_disparity
        (run_disparity / disparity / disparities serve them).  params: an SgmParams, a dict of its fields, or keyword fields
        (defaults for the rest); set_sgm(None) turns it off (the default).  One method at a time: refused while set_disparity is
        on."""
        self._set_dense(self.L.viso_batch_set_sgm, SgmParams, sgm_params, params, kw, a="an")

    def set_speckle(self, params=None, **kw):
        """viso_batch_set_speckle: the speckle filter over the batch's maps, right behind whichever method is on (set_disparity or
        set_sgm), in the next image-in runs and in run_disparity; disparity / disparities serve the filtered maps.  params: a
        SpeckleParams, a dict of its fields, or keyword fields (defaults for the rest); set_speckle(None) turns it off (the
        default).  With no method on it does nothing."""
        self._set_dense(self.L.viso_batch_set_speckle, SpeckleParams, speckle_params, params, kw)

    def disparity_points(self, t, pose=None, min_disp16=1):
        """viso_batch_get_disparity_points: frame t's resident map as an organised point image float32 [rows][cols][3], with the
        batch's calibration (set_params) and an optional 4 x 4 pose; NaNs where the pixel is invalid or below min_disp16.  Equal to
        disparity_to_points(self.disparity(t), param, pose, min_disp16).  (Batch.points is the older call for the solver's sparse
        inputs.)  With the run's trajectory:

            tr, ok, _ = batch.poses()
            poses, valid = hostmath.chain_poses(tr, ok)      # poses[k + 1] places frame valid[k] in frame 0's coordinates
            P = batch.disparity_points(valid[k], pose=poses[k + 1])
        """
        T, Tp = _pose_arg("Batch.disparity_points", pose)
        out = np.empty(tuple(self.image_shape()) + (3,), np.float32)
        _call(self.L.viso_batch_get_disparity_points, self.h, int(t), Tp, int(min_disp16), ptr(out, C.c_float))
        return out

    def _range_poses(self, where, poses, t0, t1):
        """The end of the frames t0 .. t1-1 (t1 None: to the last frame) and their poses as a contiguous float64 [t1 - t0][4][4]."""
        t1 = self.nf if t1 is None else int(t1)
        T = np.ascontiguousarray(poses, dtype=np.float64)
        if T.ndim != 3 or T.shape[1:] != (4, 4) or T.shape[0] != t1 - int(t0):
            raise ValueError(where + ": poses must be [t1 - t0][4][4]")
        return t1, T

    def fuse_disparities(self, vmap, poses, t0=0, t1=None):
        """viso_batch_fuse_disparities: the resident maps of frames t0 .. t1-1 (t1 None: to the last frame) fused into the VoxelMap
        on the device, frame t0 + i with the 4 x 4 pose poses[i]; no map is copied to the host.  The map must be on this batch's
        context."""
        t1, T = self._range_poses("Batch.fuse_disparities", poses, t0, t1)
        _call(self.L.viso_batch_fuse_disparities, self.h, vmap.h, int(t0), t1, ptr(T, C.c_double))

    def fuse_tsdf(self, tsdf, poses, t0=0, t1=None):
        """viso_batch_fuse_tsdf: the resident maps of frames t0 .. t1-1 (t1 None: to the last frame) fused into the TsdfMap on the
        device, frame t0 + i with the 4 x 4 pose poses[i]; no map is copied to the host.  The map must be on this batch's context."""
        t1, T = self._range_poses("Batch.fuse_tsdf", poses, t0, t1)
        _call(self.L.viso_batch_fuse_tsdf, self.h, tsdf.h, int(t0), t1, ptr(T, C.c_double))

    @property
    def retract_tsdf(self):
        """viso_batch_retract_tsdf (include/viso_hip.h, "TSDF retract"), called as `batch.retract_tsdf(tsdf, poses, t0=0, t1=None)`:
        the resident maps of frames t0 .. t1-1 (a gray map's with the resident left images) taken out of the TsdfMap again, frame
        t0 + i at the 4 x 4 pose poses[i] it was fused at, all in one call that stands or falls as a whole.  Returns the report as
        a dict (TsdfMap.retract); a refusal raises the library's error with it as .report and leaves the map unchanged.  A
        property that hands out the call, like TsdfMap.distance_field."""
        return lambda tsdf, poses, t0=0, t1=None: self._retract_tsdf("retract", tsdf, (poses,), t0, t1)

    @property
    def move_tsdf(self):
        """viso_batch_move_tsdf, called as `batch.move_tsdf(tsdf, old_poses, new_poses, t0=0, t1=None)`: retract_tsdf at old_poses
        and, if that is not refused, fuse_tsdf at new_poses, under one hold on the map.  Returns the retract's report."""
        return lambda tsdf, old_poses, new_poses, t0=0, t1=None: self._retract_tsdf("move", tsdf, (old_poses, new_poses), t0, t1)

    def _retract_tsdf(self, name, tsdf, poses, t0, t1):
        where = f"Batch.{name}_tsdf"
        T = [self._range_poses(where, p, t0, t1) for p in poses]
        return _reported(getattr(self.L, f"viso_batch_{name}_tsdf"), self.h, tsdf.h, int(t0), T[0][0], *(ptr(p, C.c_double) for _, p in T))

    def align_tsdf(self, tsdf, poses, t0=0, t1=None, photo=False, **params):
        """viso_batch_align_tsdf: the resident maps of frames t0 .. t1-1 (t1 None: to the last frame) aligned against the TsdfMap, each
        on its own from the 4 x 4 guess poses[i]; no map is copied to the host.  Returns a TSDF_ALIGNMENT_DTYPE array [t1 - t0], each
        what TsdfMap.align gives for that map and guess.  params: the fields of tsdf_align_params.  The map must be on this batch's
        context.
        photo=True (a gray map): viso_batch_align_tsdf_gray, with frame t's resident left image; params also takes photo_weight and
        photo_gate, and the records are TSDF_ALIGNMENT_GRAY_DTYPE ones: cost_geo, cost_photo and n_photo_used follow the fields."""
        t1, T = self._range_poses("Batch.align_tsdf", poses, t0, t1)
        if photo:
            fn, p, rec = self.L.viso_batch_align_tsdf_gray, tsdf_align_gray_params(**params), np.zeros(len(T), TSDF_ALIGNMENT_GRAY_DTYPE)
        else:
            fn, p, rec = self.L.viso_batch_align_tsdf, tsdf_align_params(**params), np.zeros(len(T), TSDF_ALIGNMENT_DTYPE)
        _call(fn, self.h, tsdf.h, int(t0), t1, ptr(T, C.c_double), C.byref(p), rec.ctypes.data)
        return rec

    def run_disparity(self):
        """viso_batch_run_disparity: only the disparity, over the resident images (upload_images_only)."""
        _call(self.L.viso_batch_run_disparity, self.h)

    def disparity(self, t):
        """Frame t's int16 map [rows][cols] from the last run that computed one."""
        out = np.empty(self.image_shape(), np.int16)
        _call(self.L.viso_batch_get_disparity, self.h, int(t), ptr(out, C.c_int16))
        return out

    def disparities(self):
        """Every frame's int16 map, [n_frames][rows][cols]."""
        out = np.empty((self.nf,) + tuple(self.image_shape()), np.int16)
        _call(self.L.viso_batch_get_disparities, self.h, ptr(out, C.c_int16))
        return out

    def _records(self, name, dtype, t=None):
        """viso_batch_get_<name>(t): frame t's record of the last run (a 0-d array of dtype), or with t None viso_batch_get_<name>s:
        the records of all frames (structured array [n_frames], frame 0: status 0)."""
        if t is None:
            out = np.zeros(self.nf, dtype)
            _call(getattr(self.L, f"viso_batch_get_{name}s"), self.h, out.ctypes.data)
        else:
            out = np.zeros((), dtype)
            _call(getattr(self.L, f"viso_batch_get_{name}"), self.h, int(t), out.ctypes.data)
        return out

    def set_covariance(self, mode, sigma=None):
        """viso_batch_set_covariance: 0 = off (default), 1 = per-frame motion covariance with sigma^2 estimated, 2 = with the given
        sigma (pixels), for the next runs (run, and run_images unless matcher_only)."""
        _call(self.L.viso_batch_set_covariance, self.h, int(mode), _sigma(sigma))

    def covariance(self, t):
        """The motion covariance record of frame t from the last run (a 0-d MOTION_COV_DTYPE array)."""
        return self._records("covariance", MOTION_COV_DTYPE, t)

    def covariances(self):
        """The records of all frames from the last run: structured array [n_frames] of MOTION_COV_DTYPE (frame 0: status 0)."""
        return self._records("covariance", MOTION_COV_DTYPE)

    def set_refine(self, mode, sigma=None):
        """viso_batch_set_refine: 0 = off (default), 1 = two-frame bundle adjustment of every solved frame with sigma^2 estimated,
        2 = with the given sigma (pixels), for the next runs (run, and run_images unless matcher_only)."""
        _call(self.L.viso_batch_set_refine, self.h, int(mode), _sigma(sigma))

    def refine(self, t):
        """The refinement record of frame t from the last run (a 0-d MOTION_REFINE_DTYPE array)."""
        return self._records("refine", MOTION_REFINE_DTYPE, t)

    def refines(self):
        """The records of all frames from the last run: structured array [n_frames] of MOTION_REFINE_DTYPE (frame 0: status 0)."""
        return self._records("refine", MOTION_REFINE_DTYPE)

    def refined_points(self, t):
        """(idx [n] int32, X [3][n] float64): frame t's used inliers and their refined points from the last run (empty unless the
        record's status is 1)."""
        idx = np.zeros(self.cap, np.int32)
        X = np.zeros((3, self.cap))
        n = C.c_int(0)
        _call(self.L.viso_batch_get_refined_points, self.h, int(t), ptr(idx, C.c_int32), ptr(X, C.c_double), C.byref(n))
        return idx[:n.value].copy(), X[:, :n.value].copy()

    def set_window_refine(self, K, mode=1, sigma=None):
        """viso_batch_set_window_refine: K = 0 off (default), K in 2..5 the sliding-window bundle adjustment of every solved frame
        over the window of frames t-K+1..t (mode 1: sigma^2 estimated, mode 2: the given sigma in pixels), for the next runs (run,
        and run_images unless matcher_only)."""
        _call(self.L.viso_batch_set_window_refine, self.h, int(K), int(mode), _sigma(sigma))

    def window_refine(self, t):
        """The window record of frame t from the last run (a 0-d WINDOW_RECORD_DTYPE array)."""
        return self._records("window_refine", WINDOW_RECORD_DTYPE, t)

    def window_refines(self):
        """The window records of all frames from the last run: structured array [n_frames] of WINDOW_RECORD_DTYPE (frame 0: status 0)."""
        return self._records("window_refine", WINDOW_RECORD_DTYPE)

    def points(self, t):
        """(X [3][m], obs [4][m]) float64: frame t's solver inputs from the last run (previous-frame points, (uL, vL, uR, vR))."""
        X = np.zeros((3, self.cap))
        obs = np.zeros((4, self.cap))
        m = C.c_int(0)
        _call(self.L.viso_batch_get_points, self.h, int(t), ptr(X, C.c_double), ptr(obs, C.c_double), C.byref(m))
        return X[:, :m.value].copy(), obs[:, :m.value].copy()

    def set_params(self, stereo, temporal, param, seed=0, first_frame=0):
        _call(self.L.viso_batch_set_params, self.h, C.byref(stereo), C.byref(temporal), C.byref(param), seed, first_frame)
        self.ransac_iter = int(param.ransac_iter)     # what viso_batch_get_hypotheses copies per frame

    def run_matcher(self):
        _call(self.L.viso_batch_run_matcher, self.h)

    def run(self):
        _call(self.L.viso_batch_run, self.h)

    def matches(self, which, t):
        out = np.empty((self.cap, 3), np.int32)
        n = C.c_int(0)
        _call(self.L.viso_batch_get_matches, self.h, which, t, ptr(out, C.c_int32), C.byref(n))
        return out[:n.value].copy()

    def circle(self, t):
        circ = np.empty((self.cap, 4), np.int32)
        pcl = np.empty((self.cap, 2), np.int32)
        n = C.c_int(0)
        _call(self.L.viso_batch_get_circle, self.h, t, ptr(circ, C.c_int32), ptr(pcl, C.c_int32), C.byref(n))
        return circ[:n.value].copy(), pcl[:n.value].copy()

    def pose(self, t):
        tr = np.zeros(6)
        ok, n = C.c_int(0), C.c_int(0)
        inl = np.empty(self.cap, np.int32)
        _call(self.L.viso_batch_get_pose, self.h, t, ptr(tr, C.c_double), C.byref(ok), ptr(inl, C.c_int32), C.byref(n))
        return ok.value, tr, inl[:n.value].copy()

    def poses(self):
        tr = np.zeros((self.nf, 6))
        ok = np.zeros(self.nf, np.int32)
        n = np.zeros(self.nf, np.int32)
        _call(self.L.viso_batch_get_poses, self.h, ptr(tr, C.c_double), ptr(ok, C.c_int32), ptr(n, C.c_int32))
        return tr, ok, n

    def hypotheses(self, iters=None):
        """(tr_h [nf][iters][6], ok_h [nf][iters], cnt_h [nf][iters], n_undecided) of the last run's RANSAC stage.
        The buffers are sized from the ransac_iter given to set_params (the library copies nf * that many entries);
        an `iters` that disagrees is refused instead of letting the copy run past a smaller buffer."""
        have = getattr(self, "ransac_iter", None)
        if have is None:
            raise RuntimeError("hypotheses(): set_params has not been called on this batch")
        if iters is not None and iters != have:
            raise ValueError(f"hypotheses(iters={iters}): the batch was set up with ransac_iter={have}")
        iters = have
        tr = np.zeros((self.nf, iters, 6))
        ok = np.zeros((self.nf, iters), np.int32)
        cnt = np.zeros((self.nf, iters), np.int32)
        nu = np.zeros(1, np.int32)
        _call(self.L.viso_batch_get_hypotheses, self.h, ptr(tr, C.c_double), ptr(ok, C.c_int32), ptr(cnt, C.c_int32), ptr(nu, C.c_int32))
        return tr, ok, cnt, int(nu[0])

    def counters(self):
        sc = np.zeros((3, self.nf), np.int64)
        mo = np.zeros((3, self.nf), np.int64)
        _call(self.L.viso_batch_get_counters, self.h, ptr(sc, C.c_int64), ptr(mo, C.c_int64))
        return sc, mo

    def general_path_flags(self):
        f = np.zeros((self.nf, 2), np.int32)
        _call(self.L.viso_batch_get_general_path_flags, self.h, ptr(f, C.c_int32))
        return f

    def overflow_count(self):
        n = C.c_int32(0)
        _call(self.L.viso_batch_get_overflow_count, self.h, C.byref(n))
        return n.value

    def row8_shift(self):
        s = C.c_int(-1)
        _call(self.L.viso_batch_get_row8_shift, self.h, C.byref(s))
        return s.value

    def kernel_timing(self, enable):
        _call(self.L.viso_batch_kernel_timing, self.h, int(enable))

    def kernel_ms(self):
        ms = C.c_double(0)
        n = C.c_int(0)
        _call(self.L.viso_batch_kernel_ms, self.h, C.byref(ms), C.byref(n))
        return ms.value, n.value

    def device_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _call(self.L.viso_batch_device_ptrs, self.h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value
