"""The plain (host-pointer) family of include/viso_hip.h under the reference's names, the Harris detector, the descriptor
extraction and the sub-pixel refinement of stereo matches: numpy in, numpy out, one call of csrc/plain.hip each."""
import ctypes as C

import numpy as np

from . import _call, _f32, _f64, _fail, _i32, _image_pair, load
from .abi import ptr

HARRIS_K = float(np.float32(0.04))   # the reference's intended default (float k = .04, src/viso.cpp:915)


def match_desc(kp1, kp2, d1, d2, mp):
    """match_desc, reference src/viso.cpp:669-726 -> (M,3) int32 (i1,i2,dist)."""
    L = load()
    kp1, kp2 = _f32(kp1).reshape(-1, 2), _f32(kp2).reshape(-1, 2)
    d1, d2 = _f32(d1), _f32(d2)
    n1, n2 = len(kp1), len(kp2)
    dlen = d1.shape[1] if d1.ndim == 2 else d2.shape[1]
    out = np.empty((max(n1, 1), 3), np.int32)
    n = C.c_int(0)
    _call(L.viso_match_desc, ptr(kp1, C.c_float), n1, ptr(kp2, C.c_float), n2, ptr(d1, C.c_float),
          ptr(d2, C.c_float), dlen, C.byref(mp), ptr(out, C.c_int32), C.byref(n))
    return out[:n.value].copy()


def match_circle(lr, lr_prev, m11, m22, cap=None):
    L = load()
    lr, lr_prev, m11, m22 = (_i32(a).reshape(-1, 3) for a in (lr, lr_prev, m11, m22))
    cap = cap if cap is not None else max(1, len(lr) * 4)
    circ = np.empty((cap, 4), np.int32)
    pcl = np.empty((cap, 2), np.int32)
    n = C.c_int(0)
    r = L.viso_match_circle(ptr(lr, C.c_int32), len(lr), ptr(lr_prev, C.c_int32), len(lr_prev),
                            ptr(m11, C.c_int32), len(m11), ptr(m22, C.c_int32), len(m22),
                            ptr(circ, C.c_int32), ptr(pcl, C.c_int32), cap, C.byref(n))
    if r < 0 and r != -1:
        _fail(L.viso_match_circle, r)
    k = min(n.value, cap)
    return r, circ[:k].copy(), pcl[:k].copy(), n.value


def collect_matches(kp1, kp2, match):
    L = load()
    kp1, kp2 = _f32(kp1).reshape(-1, 2), _f32(kp2).reshape(-1, 2)
    match = _i32(match).reshape(-1, 3)
    x = np.empty((4, len(match)), np.float64)
    _call(L.viso_collect_matches, ptr(kp1, C.c_float), len(kp1), ptr(kp2, C.c_float), len(kp2),
          ptr(match, C.c_int32), len(match), ptr(x, C.c_double))
    return x


def triangulate_rectified(x, param):
    L = load()
    x = _f64(x)
    X = np.empty((3, x.shape[1]), np.float64)
    _call(L.viso_triangulate_rectified, ptr(x, C.c_double), x.shape[1], C.byref(param), ptr(X, C.c_double))
    return X


def minimize_reproj(X, obs, tr, param, active):
    L = load()
    X, obs, active = _f64(X), _f64(obs), _i32(active)
    tr = _f64(tr).copy()
    r = L.viso_minimize_reproj(ptr(X, C.c_double), ptr(obs, C.c_double), X.shape[1],
                               ptr(tr, C.c_double), C.byref(param), ptr(active, C.c_int32), len(active))
    if r < 0:
        _fail(L.viso_minimize_reproj, r)
    return r, tr


def get_inliers(X, obs, tr, param):
    L = load()
    X, obs, tr = _f64(X), _f64(obs), _f64(tr)
    m = X.shape[1]
    inl = np.empty(max(m, 1), np.int32)
    n = C.c_int(0)
    rms = C.c_double(0)
    _call(L.viso_get_inliers, ptr(X, C.c_double), ptr(obs, C.c_double), m, ptr(tr, C.c_double),
          C.byref(param), ptr(inl, C.c_int32), C.byref(n), C.byref(rms))
    return inl[:n.value].copy(), rms.value


def support_sizes(X, obs, tr_h, param):
    """Support size of every motion tr_h[k] over (X, obs), through the RANSAC stage's counting kernel."""
    L = load()
    X, obs, tr_h = _f64(X), _f64(obs), _f64(np.atleast_2d(tr_h))
    cnt = np.zeros(max(len(tr_h), 1), np.int32)
    _call(L.viso_support_sizes, ptr(X, C.c_double), ptr(obs, C.c_double), X.shape[1], ptr(tr_h, C.c_double), len(tr_h),
          C.byref(param), ptr(cnt, C.c_int32))
    return cnt[:len(tr_h)].copy()


def ransac_samples(seed, frame, iters, m):
    out = np.empty((iters, 3), np.int32)
    load().viso_ransac_samples(seed, frame, iters, m, ptr(out, C.c_int32))
    return out


def ransac_minimize_reproj(X, obs, param, samples=None, seed=0, frame=0, tr0=None):
    L = load()
    X, obs = _f64(X), _f64(obs)
    m = X.shape[1]
    tr = np.zeros(6) if tr0 is None else _f64(tr0).copy()
    inl = np.empty(max(m, 1), np.int32)
    n = C.c_int(0)
    s = None if samples is None else _i32(samples)
    r = L.viso_ransac_minimize_reproj(ptr(X, C.c_double), ptr(obs, C.c_double), m, ptr(tr, C.c_double),
                                      ptr(inl, C.c_int32), C.byref(n), C.byref(param),
                                      ptr(s, C.c_int32), seed, frame)
    if r < 0:
        _fail(L.viso_ransac_minimize_reproj, r)
    return r, tr, inl[:n.value].copy()


def tr2mat(tr):
    tr = _f64(tr)
    T = np.empty((4, 4))
    load().viso_tr2mat(ptr(tr, C.c_double), ptr(T, C.c_double))
    return T


def pose_update(pose, tr):
    pose, tr = _f64(pose), _f64(tr)
    out = np.empty((4, 4))
    load().viso_pose_update(ptr(pose, C.c_double), ptr(tr, C.c_double), ptr(out, C.c_double))
    return out


def F_from_P(P1, P2):
    P1, P2 = _f64(P1), _f64(P2)
    F = np.empty((3, 3))
    load().viso_F_from_P(ptr(P1, C.c_double), ptr(P2, C.c_double), ptr(F, C.c_double))
    return F


def extract_descriptors(img, kp, radius=5):
    """MyFeatureExtractor::computeImpl, reference src/viso.cpp:1004-1024."""
    L = load()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    kp = _f32(kp).reshape(-1, 2)
    d = np.empty((len(kp), (2 * radius + 1) ** 2), np.float32)
    _call(L.viso_extract_descriptors, ptr(img, C.c_uint8), img.shape[0], img.shape[1], ptr(kp, C.c_float),
          len(kp), radius, ptr(d, C.c_float))
    return d


def refine_stereo_subpixel(imgL, imgR, kp1, kp2, match, mode=1):
    """viso_refine_stereo_subpixel: the opt-in sub-pixel refinement of stereo matches (not in the reference;
    include/viso_hip.h).  match: (n, 3) int32 rows (i1, i2, dist) into kp1 / kp2; mode 1 (horizontal) or 2 (both axes).
    Returns (n, 2) float32 refined right-image points (uR', vR')."""
    L = load()
    imgL, imgR = _image_pair("refine_stereo_subpixel", imgL, imgR)
    kp1, kp2 = _f32(kp1).reshape(-1, 2), _f32(kp2).reshape(-1, 2)
    match = _i32(match).reshape(-1, 3)
    out = np.empty((max(len(match), 1), 2), np.float32)
    _call(L.viso_refine_stereo_subpixel, ptr(imgL, C.c_uint8), ptr(imgR, C.c_uint8), imgL.shape[0], imgL.shape[1],
          ptr(kp1, C.c_float), len(kp1), ptr(kp2, C.c_float), len(kp2),
          ptr(match, C.c_int32), len(match), int(mode), ptr(out, C.c_float))
    return out[:len(match)].copy()


def harris_response(img, k=HARRIS_K):
    """cv::cornerHarris(img, R, 3, 5, k, BORDER_DEFAULT) restated (reference src/viso.cpp:930)."""
    L = load()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    r = np.empty(img.shape, np.float32)
    _call(L.viso_harris_response, ptr(img, C.c_uint8), img.shape[0], img.shape[1], k, ptr(r, C.c_float))
    return r


def detect_harris_binned(img, n_features=1200, nbinx=24, nbiny=5, k=HARRIS_K):
    """HarrisBinnedFeatureDetector::detectImpl, reference src/viso.cpp:926-975."""
    L = load()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    kp = np.empty((max(1, n_features), 2), np.float32)
    resp = np.empty(max(1, n_features), np.float32)
    n = C.c_int(0)
    _call(L.viso_detect_harris_binned, ptr(img, C.c_uint8), img.shape[0], img.shape[1], n_features, nbinx, nbiny, k,
          ptr(kp, C.c_float), ptr(resp, C.c_float), C.byref(n))
    return kp[:n.value].copy(), resp[:n.value].copy()
