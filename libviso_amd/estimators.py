"""The three fp64 motion estimators of include/viso_hip.h as direct calls (csrc/batch_estimators.hip): the motion covariance, the
two-frame and the sliding-window bundle adjustment, and the propagation of their covariances along a trajectory."""
import ctypes as C

import numpy as np

from . import _call, _f64, _i32, _sigma, load
from .abi import MOTION_COV_DTYPE, MOTION_REFINE_DTYPE, WINDOW_RECORD_DTYPE, ptr


def _pose_inputs(where, X, obs, tr, inliers):
    """The direct calls' inputs as contiguous arrays (X 3 x m, obs 4 x m, tr 6 float64; the inlier list int32), and m."""
    X, obs, tr, inl = _f64(X), _f64(obs), _f64(tr), _i32(inliers)
    if X.ndim != 2 or X.shape[0] != 3 or obs.shape != (4, X.shape[1]) or tr.shape != (6,):
        raise ValueError(f"{where}: X must be (3, m), obs (4, m) and tr (6,); got {X.shape}, {obs.shape}, {tr.shape}")
    return X, obs, tr, inl, X.shape[1]


def pose_covariance(X, obs, tr, inliers, param, mode=1, sigma=None):
    """viso_pose_covariance: the motion covariance record (a 0-d MOTION_COV_DTYPE array) of one frame's solve -- X 3 x m, obs 4 x m,
    tr 6, inliers the final inlier list; mode 1 estimates sigma^2, mode 2 takes sigma (pixels)."""
    L = load()
    X, obs, tr, inl, m = _pose_inputs("pose_covariance", X, obs, tr, inliers)
    out = np.zeros((), MOTION_COV_DTYPE)
    _call(L.viso_pose_covariance, ptr(X, C.c_double), ptr(obs, C.c_double), m, ptr(tr, C.c_double), ptr(inl, C.c_int32), len(inl),
          C.byref(param), int(mode), _sigma(sigma), out.ctypes.data)
    return out


def pose_refine(X, obs, tr, inliers, param, mode=1, sigma=None):
    """viso_pose_refine: the two-frame bundle adjustment of one frame's solve -- X 3 x m, obs 4 x m, tr 6, inliers the final inlier
    list; mode 1 estimates sigma^2, mode 2 takes sigma (pixels).  Returns (record, points): a 0-d MOTION_REFINE_DTYPE array and
    the refined points (3, n) in the order of the used inliers (empty unless status is 1)."""
    L = load()
    X, obs, tr, inl, m = _pose_inputs("pose_refine", X, obs, tr, inliers)
    out = np.zeros((), MOTION_REFINE_DTYPE)
    pts = np.zeros((3, max(len(inl), 1)))
    _call(L.viso_pose_refine, ptr(X, C.c_double), ptr(obs, C.c_double), m, ptr(tr, C.c_double), ptr(inl, C.c_int32), len(inl),
          C.byref(param), int(mode), _sigma(sigma), out.ctypes.data, ptr(pts, C.c_double))
    k = int(out["n"]) if int(out["status"]) == 1 else 0
    return out, pts[:, :k].copy()


def refines_as_covariances(recs):
    """Refine records packed as MOTION_COV_DTYPE (cov, sigma2, gap, status, n; delta zero), so that
    chain_covariances(recs["tr"], ok, refines_as_covariances(recs)) propagates the refined trajectory's uncertainty."""
    recs = np.asarray(recs, MOTION_REFINE_DTYPE)
    out = np.zeros(recs.shape, MOTION_COV_DTYPE)
    for k in ("cov", "sigma2", "gap", "status", "n"):
        out[k] = recs[k]
    return out


def window_refine(frames, param, mode=1, sigma=None):
    """viso_window_refine: the sliding-window bundle adjustment's record of the last frame of a window of len = len(frames) + 1
    frames (2..5), K = len.  frames: the window's frames 1..len-1, oldest first, each a tuple (X 3 x m, obs 4 x m, left m x 2 of
    (cur-left, prev-left) keypoint indices, tr 6, inliers); frame 0's rows are never used.  mode 1 estimates sigma^2, mode 2 takes
    sigma (pixels).  Returns a 0-d WINDOW_RECORD_DTYPE array."""
    L = load()
    Xs, Os, Ls, Ts, Is, ms, ns = [], [], [], [], [], [], []
    for X, obs, left, tr, inl in frames:
        X, obs, tr, inl = _f64(X), _f64(obs), _f64(tr), _i32(inl)
        left = np.ascontiguousarray(np.asarray(left, np.int32).reshape(-1, 2))
        if X.ndim != 2 or X.shape[0] != 3 or obs.shape != (4, X.shape[1]) or tr.shape != (6,) or left.shape[0] != X.shape[1]:
            raise ValueError(f"window_refine: X must be (3, m), obs (4, m), left (m, 2) and tr (6,); got {X.shape}, {obs.shape}, "
                             f"{left.shape}, {tr.shape}")
        Xs.append(X.ravel()); Os.append(obs.ravel()); Ls.append(left.ravel()); Ts.append(tr); Is.append(inl)
        ms.append(X.shape[1]); ns.append(len(inl))
    cat = lambda a, dt: np.ascontiguousarray(np.concatenate(a) if a else np.zeros(0), dt)   # noqa: E731
    X, obs, left, inl = cat(Xs, np.float64), cat(Os, np.float64), cat(Ls, np.int32), cat(Is, np.int32)
    tr = np.ascontiguousarray(np.array(Ts, np.float64).reshape(-1, 6))
    m, n = np.ascontiguousarray(ms, np.intc), np.ascontiguousarray(ns, np.intc)
    out = np.zeros((), WINDOW_RECORD_DTYPE)
    _call(L.viso_window_refine, len(frames) + 1, ptr(m, C.c_int), ptr(X, C.c_double), ptr(obs, C.c_double), ptr(left, C.c_int32),
          ptr(tr, C.c_double), ptr(inl, C.c_int32), ptr(n, C.c_int), C.byref(param), int(mode), _sigma(sigma), out.ctypes.data)
    return out


def window_refines_as_covariances(recs):
    """Window records packed as MOTION_COV_DTYPE (cov, sigma2, gap, status; n = n_points; delta zero), so that
    chain_covariances(recs["tr"], ok, window_refines_as_covariances(recs)) propagates the refined trajectory's uncertainty."""
    recs = np.asarray(recs, WINDOW_RECORD_DTYPE)
    out = np.zeros(recs.shape, MOTION_COV_DTYPE)
    for k in ("cov", "sigma2", "gap", "status"):
        out[k] = recs[k]
    out["n"] = recs["n_points"]
    return out


def chain_covariances(tr, ok, covs):
    """viso_chain_covariances (host only): (pose_cov [k][6][6], valid [k]) along hostmath.chain_poses' list, k = 1 + sum(ok != 0)."""
    L = load()
    tr, ok = _f64(np.reshape(tr, (-1, 6))), _i32(ok)
    covs = np.ascontiguousarray(covs, MOTION_COV_DTYPE)
    n = len(tr)
    if len(ok) != n or len(covs) != n:
        raise ValueError("chain_covariances: tr, ok and covs need one entry per frame")
    out = np.zeros((n + 1, 6, 6))
    valid = np.zeros(n + 1, np.int32)
    k = C.c_int(0)
    _call(L.viso_chain_covariances, ptr(tr, C.c_double), ptr(ok, C.c_int32), covs.ctypes.data, n, ptr(out, C.c_double),
          ptr(valid, C.c_int32), C.byref(k))
    return out[:k.value].copy(), valid[:k.value].copy()
