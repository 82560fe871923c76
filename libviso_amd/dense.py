"""The dense stage of include/viso_hip.h as direct calls (csrc/batch_dense.hip): rectification of raw images, block matching,
semi-global matching, the speckle filter and the reprojection of a disparity map to points."""
import ctypes as C

import numpy as np

from . import _call, _f32, _f64, _image_pair, _map16, _params, _pose_arg, load
from .abi import SGM_DEFAULTS, SPECKLE_DEFAULTS, DisparityParams, SgmParams, SpeckleParams, ptr

DISP_INVALID = -16   # VISO_DISP_INVALID


def rectify_map(K, D, R, P, out_shape):
    """viso_rectify_map: the map of one camera (opt-in rectification, not in the reference; include/viso_hip.h), on the host.
    K 3x3 (K[0][1] == 0), D (k1, k2, p1, p2, k3), R 3x3 rectifying rotation, P 3x4 rectified projection; out_shape (rows, cols).
    Returns (mapx, mapy), float32 arrays of out_shape: the raw-image position every output pixel samples."""
    L = load()
    K, D, R, P = (_f64(np.asarray(a, np.float64).reshape(-1)) for a in (K, D, R, P))
    if (K.size, D.size, R.size, P.size) != (9, 5, 9, 12):
        raise ValueError("rectify_map: K 3x3, D 5, R 3x3, P 3x4")
    rows, cols = (int(v) for v in out_shape)
    mapx = np.empty((max(rows, 1), max(cols, 1)), np.float32)
    mapy = np.empty_like(mapx)
    _call(L.viso_rectify_map, ptr(K, C.c_double), ptr(D, C.c_double), ptr(R, C.c_double), ptr(P, C.c_double), rows, cols,
          ptr(mapx, C.c_float), ptr(mapy, C.c_float))
    return mapx, mapy


def _map_pair(mapx, mapy, out_shape):
    mapx, mapy = _f32(mapx), _f32(mapy)
    if mapx.shape != tuple(out_shape) or mapy.shape != tuple(out_shape):
        raise ValueError(f"maps must have the output shape {tuple(out_shape)}")
    return mapx, mapy


def rectify_images(raw, mapx, mapy, out_shape, border=0):
    """viso_rectify_images: raw uint8 images (n, raw_rows, raw_cols) or one (raw_rows, raw_cols) of ONE camera -> rectified images
    of out_shape, on the device (the batch's kernel; the remap rule of include/viso_hip.h)."""
    L = load()
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    single = raw.ndim == 2
    if single:
        raw = raw[None]
    n, rr, rc = raw.shape
    rows, cols = (int(v) for v in out_shape)
    mapx, mapy = _map_pair(mapx, mapy, (rows, cols))
    out = np.empty((max(n, 1), rows, cols), np.uint8)
    _call(L.viso_rectify_images, ptr(raw, C.c_uint8), n, rr, rc, ptr(mapx, C.c_float), ptr(mapy, C.c_float), rows, cols, int(border),
          ptr(out, C.c_uint8))
    return out[0].copy() if single else out[:n].copy()


def disparity_params(**params):
    """viso_disparity_params: viso_disparity_params_default with the given fields (num_disp, block, prefilter_cap,
    texture_threshold, uniqueness, lr_max_diff) replaced."""
    p = DisparityParams()
    load().viso_disparity_params_default(C.byref(p))
    for k, v in params.items():
        if k not in dict(DisparityParams._fields_):
            raise TypeError(f"disparity_params: unknown parameter {k!r}")
        setattr(p, k, int(v))
    return p


def stereo_disparity(imgL, imgR, **params):
    """viso_stereo_disparity: the dense disparity map of one rectified pair (opt-in, not in the reference; the definition of
    include/viso_hip.h), on the device.  Returns int16 [rows][cols] in 1/16 px, DISP_INVALID where invalid."""
    L = load()
    imgL, imgR = _image_pair("stereo_disparity", imgL, imgR)
    p = disparity_params(**params)
    out = np.empty(imgL.shape, np.int16)
    _call(L.viso_stereo_disparity, ptr(imgL, C.c_uint8), ptr(imgR, C.c_uint8), imgL.shape[0], imgL.shape[1], C.byref(p),
          ptr(out, C.c_int16))
    return out


def sgm_params(**params):
    """viso_sgm_params: viso_sgm_params_default with the given fields (num_disp, p1, p2, paths, uniqueness, lr_max_diff) replaced.
    Needs no library: the ranges are checked by the calls that take it (SgmParams.ok restates them)."""
    return _params(SgmParams, SGM_DEFAULTS, "sgm_params", params)


def stereo_sgm(imgL, imgR, **params):
    """viso_stereo_sgm: the dense disparity map of one rectified pair by semi-global matching (opt-in, not in the reference; the
    definition of include/viso_hip.h), on the device.  Returns int16 [rows][cols] in 1/16 px, DISP_INVALID where invalid."""
    L = load()
    imgL, imgR = _image_pair("stereo_sgm", imgL, imgR)
    p = sgm_params(**params)
    out = np.empty(imgL.shape, np.int16)
    _call(L.viso_stereo_sgm, ptr(imgL, C.c_uint8), ptr(imgR, C.c_uint8), imgL.shape[0], imgL.shape[1], C.byref(p), ptr(out, C.c_int16))
    return out


def sgm_set_workspace_cap(nbytes):
    """viso_sgm_set_workspace_cap: the bytes of census words and S volumes one group of frames may take (0: the default)."""
    load().viso_sgm_set_workspace_cap(int(nbytes))


def sgm_frame_bytes(rows, cols, num_disp=128):
    """The workspace of one frame: the two images' census words and the S volume, each rounded up to 256 bytes."""
    up = lambda b: (b + 255) & ~255   # noqa: E731
    return up(rows * cols * 16) + up(rows * cols * num_disp * 2)


def speckle_params(**params):
    """viso_speckle_params: viso_speckle_params_default with the given fields (max_size in pixels, max_diff in 1/16 px) replaced.
    Needs no library: the ranges are checked by the calls that take it (SpeckleParams.ok restates them)."""
    return _params(SpeckleParams, SPECKLE_DEFAULTS, "speckle_params", params)


def filter_speckles(d16, **params):
    """viso_filter_speckles: a copy of the int16 map with every 4-connected component of at most max_size pixels (neighbours linked
    when they differ by at most max_diff) set to DISP_INVALID (opt-in, not in the reference; the definition of include/viso_hip.h),
    on the device."""
    out = _map16("filter_speckles", d16).copy()
    p = speckle_params(**params)
    _call(load().viso_filter_speckles, ptr(out, C.c_int16), out.shape[0], out.shape[1], C.byref(p))
    return out


def speckle_set_workspace_cap(nbytes):
    """viso_speckle_set_workspace_cap: the bytes of label and size words one group of frames may take (0: the default)."""
    load().viso_speckle_set_workspace_cap(int(nbytes))


def speckle_frame_bytes(rows, cols):
    """The workspace of one frame: a label word and a size word per pixel, each plane rounded up to 256 bytes."""
    return 2 * ((rows * cols * 4 + 255) & ~255)


def disparity_to_points(d16, param, pose=None, min_disp16=1):
    """viso_disparity_to_points: the int16 map as an organised point image float32 [rows][cols][3] (X, Y, Z in the left camera's
    frame, or transformed by the 4 x 4 pose), three NaNs where the pixel is invalid or its disparity is below min_disp16 (1/16 px).
    param: a Param (f, cu, cv, base).  A point set is `P[np.isfinite(P[..., 2])]`.  With a trajectory:

        poses, valid = hostmath.chain_poses(tr, ok)      # poses[k + 1] places frame valid[k] in frame 0's coordinates
        P = disparity_to_points(batch.disparity(valid[k]), param, pose=poses[k + 1])
    """
    d16 = _map16("disparity_to_points", d16)
    T, Tp = _pose_arg("disparity_to_points", pose)
    out = np.empty(d16.shape + (3,), np.float32)
    _call(load().viso_disparity_to_points, ptr(d16, C.c_int16), d16.shape[0], d16.shape[1], C.byref(param), Tp, int(min_disp16),
          ptr(out, C.c_float))
    return out


def disparity_to_float(d16):
    """float32 disparity in pixels (d16 / 16), NaN where invalid."""
    d16 = np.asarray(d16)
    out = d16.astype(np.float32) / np.float32(16)
    out[d16 == DISP_INVALID] = np.nan
    return out
