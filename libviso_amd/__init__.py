"""libviso_amd — MI355X (gfx950) implementation of libviso's per-frame hot path.

The product is the C-ABI shared library built from libviso_amd/csrc
(libviso_hip.so, declared in include/viso_hip.h) plus the C++ host mirror of
the reference interface in libviso_amd/host.  This Python package is plumbing
for tests and bench.py: a ctypes loader and numpy-in/numpy-out wrappers with
the reference's function names.  There is NO CPU fallback: if the library is
missing, or no HIP device is present, calls raise.
"""
import atexit
import ctypes as C
import os
import subprocess
import sys
import weakref

import numpy as np

from .abi import (DESC_LEN, MAP_DEFAULTS, MAP_ENTRY_DTYPE, MapCounters, MapParams, declare_map, MOTION_COV_DTYPE, MOTION_REFINE_DTYPE, SGM_DEFAULTS, SPECKLE_DEFAULTS, WINDOW_RECORD_DTYPE, DisparityParams, MatchParams,
                  Param, SgmParams, SpeckleParams, declare_common, declare_covariance, declare_disparity, declare_refine, declare_rectify,
                  declare_sgm, declare_speckle, declare_subpixel, declare_window, f32p, f64p, i32p, i64p, intp, ptr,
                  TSDF_CROSSING_DTYPE, TSDF_DEFAULTS, TSDF_ENTRY_DTYPE, TSDF_GRAY_ENTRY_DTYPE, TSDF_MESH_VERTEX_DTYPE, TsdfCounters, TsdfParams,
                  declare_tsdf, TSDF_ALIGN_DEFAULTS, TSDF_ALIGN_STEP_DTYPE, TSDF_ALIGNMENT_DTYPE, TSDF_NORMAL_COUNTERS, TSDF_NORMAL_DTYPE,
                  TsdfAlignParams, VoxelBox, declare_evict, TSDF_ALIGN_GRAY_DEFAULTS, TSDF_ALIGN_GRAY_STEP_DTYPE, TSDF_ALIGNMENT_GRAY_DTYPE,
                  TSDF_NORMAL_GRAY_COUNTERS, TSDF_NORMAL_GRAY_DTYPE, TsdfAlignGrayParams)

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("VISO_HIP_SO") or os.path.join(_HERE, "libviso_hip.so")   # VISO_HIP_SO: another build of the library (A/B runs)
CSRC = os.path.join(_HERE, "csrc")


class VisoError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j", "6"] + (["-B"] if force else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise VisoError("building libviso_hip.so failed")
    return SO_PATH


_lib = None


def load():
    """ctypes handle of libviso_hip.so; raises when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise VisoError(f"{SO_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(there is no CPU fallback)")
    try:
        # torch ships its own libamdhip64 (same soname): load it first so this
        # process holds exactly one HIP runtime and pointers/streams can be shared.
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional plumbing
        pass
    L = C.CDLL(SO_PATH)
    MP, PP = declare_common(L, "viso_")
    L.viso_last_error.restype = C.c_char_p
    L.viso_version.restype = C.c_char_p
    L.viso_ctx_matcher_kernel_name.restype = C.c_char_p
    L.viso_ctx_matcher_kernel_name.argtypes = [C.c_void_p]
    L.viso_ctx_set_matcher.argtypes = [C.c_void_p, C.c_int]
    L.viso_matcher_variants.argtypes = [C.POINTER(C.c_int), C.c_int]
    L.viso_ctx_set_gn_split.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "viso_ctx_set_row8_shift"):   # (absent from older builds of the library: VISO_HIP_SO A/B runs)
        L.viso_ctx_set_row8_shift.argtypes = [C.c_void_p, C.c_int]
        L.viso_batch_get_row8_shift.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.viso_batch_get_hypotheses.argtypes = [C.c_void_p, f64p, i32p, i32p, i32p]
    L.viso_host_alloc.restype = C.c_void_p
    L.viso_host_alloc.argtypes = [C.c_size_t]
    L.viso_host_free.argtypes = [C.c_void_p]
    L.viso_batch_upload_async.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p, f32p, i32p]
    L.viso_batch_upload_images_async.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int,
                                                 f32p, i32p]
    L.viso_batch_upload_i16.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p, C.POINTER(C.c_int16), i32p]
    L.viso_batch_upload_i16_async.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p, C.POINTER(C.c_int16), i32p]
    L.viso_match_desc.restype = C.c_int
    L.viso_match_desc.argtypes = [f32p, C.c_int, f32p, C.c_int, f32p, f32p, C.c_int, MP, i32p, intp]
    L.viso_minimize_reproj.restype = C.c_int
    L.viso_minimize_reproj.argtypes = [f64p, f64p, C.c_int, f64p, PP, i32p, C.c_int]
    L.viso_match_params_stereo.argtypes = [MP, f64p]
    L.viso_match_params_temporal.argtypes = [MP]
    L.viso_param_default.argtypes = [PP]
    L.viso_ctx_create.restype = C.c_void_p
    L.viso_ctx_create.argtypes = [C.c_int, C.c_void_p]
    L.viso_ctx_destroy.argtypes = [C.c_void_p]
    L.viso_ctx_stream.restype = C.c_void_p
    L.viso_ctx_stream.argtypes = [C.c_void_p]
    L.viso_ctx_synchronize.argtypes = [C.c_void_p]
    L.viso_batch_create.restype = C.c_void_p
    L.viso_batch_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.viso_batch_destroy.argtypes = [C.c_void_p]
    L.viso_batch_upload.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p, f32p, i32p]
    L.viso_batch_device_ptrs.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                         C.POINTER(C.c_void_p)]
    L.viso_batch_set_params.argtypes = [C.c_void_p, MP, MP, PP, C.c_uint64, C.c_uint64]
    L.viso_batch_run_matcher.argtypes = [C.c_void_p]
    L.viso_batch_run.argtypes = [C.c_void_p]
    L.viso_batch_get_matches.argtypes = [C.c_void_p, C.c_int, C.c_int, i32p, intp]
    L.viso_batch_get_circle.argtypes = [C.c_void_p, C.c_int, i32p, i32p, intp]
    L.viso_batch_get_pose.argtypes = [C.c_void_p, C.c_int, f64p, intp, i32p, intp]
    L.viso_batch_get_poses.argtypes = [C.c_void_p, f64p, i32p, i32p]
    L.viso_batch_get_counters.argtypes = [C.c_void_p, i64p, i64p]
    L.viso_batch_get_general_path_flags.argtypes = [C.c_void_p, i32p]
    L.viso_batch_get_overflow_count.argtypes = [C.c_void_p, i32p]
    L.viso_batch_kernel_timing.argtypes = [C.c_void_p, C.c_int]
    L.viso_batch_kernel_ms.argtypes = [C.c_void_p, f64p, intp]
    L.viso_batch_upload_images.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_int, C.c_int,
                                           f32p, i32p]
    L.viso_batch_run_images.argtypes = [C.c_void_p, C.c_int]
    L.viso_batch_detect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double]
    L.viso_batch_get_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_int, f32p, intp]
    if hasattr(L, "viso_batch_set_subpixel"):   # (absent from older builds of the library: VISO_HIP_SO A/B runs)
        declare_subpixel(L)
    if hasattr(L, "viso_batch_set_rectify"):
        declare_rectify(L)
    if hasattr(L, "viso_batch_set_covariance"):
        declare_covariance(L)
    if hasattr(L, "viso_batch_set_refine"):
        declare_refine(L)
    if hasattr(L, "viso_batch_set_window_refine"):
        declare_window(L)
    if hasattr(L, "viso_batch_set_disparity"):
        declare_disparity(L)
    if hasattr(L, "viso_batch_set_sgm"):
        declare_sgm(L)
    if hasattr(L, "viso_batch_set_speckle"):
        declare_speckle(L)
    if hasattr(L, "viso_map_create"):
        declare_map(L)
    if hasattr(L, "viso_tsdf_create"):
        declare_tsdf(L)
    if hasattr(L, "viso_map_evict"):
        declare_evict(L)
    L.viso_harris_response.argtypes = [C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_double, f32p]
    L.viso_detect_harris_binned.argtypes = [C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_double, f32p, f32p, intp]
    _lib = L
    return L


def _err(where, code):
    msg = load().viso_last_error().decode(errors="replace")
    raise VisoError(f"{where} failed with {code}: {msg}")


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _sigma(sigma):
    """The sigma_px argument of the estimators: 0.0 when not given (mode 1 ignores it)."""
    return float(sigma) if sigma is not None else 0.0




def matcher_variants():
    """What this build of libviso_hip.so offers (viso_ctx_set_matcher): (3, 5, 6) for the product build —
    match_union_kernel, match_prune_kernel and match_union8_kernel (6, the default) — and (2, 3, 4, 5, 6) for
    `make DEBUG_VARIANTS=1`.  Asked of the library itself, so a debug build gets its variants tested."""
    out = (C.c_int * 8)()
    n = load().viso_matcher_variants(out, 8)
    return tuple(out[i] for i in range(min(n, 8)))


def __getattr__(name):   # MATCHER_VARIANTS / DEFAULT_MATCHER: resolved on first use (need the library, not a device)
    if name == "MATCHER_VARIANTS":
        return matcher_variants()
    if name == "DEFAULT_MATCHER":   # the build's default, or $VISO_MATCHER (viso_matcher_default)
        L = load()   # builds older than viso_matcher_default (VISO_HIP_SO A/B runs) started every context with variant 3
        return int(L.viso_matcher_default()) if hasattr(L, "viso_matcher_default") else 3
    raise AttributeError(name)


def set_matcher_variant(v, ctx=None):
    """Which kernel takes the temporal calls: of `ctx`, or of the plain family's default context."""
    r = load().viso_ctx_set_matcher(ctx.h if ctx is not None else None, int(v))
    if r != 1:
        _err("viso_ctx_set_matcher", r)


def set_row8_shift(shift, ctx=None):
    """viso_ctx_set_row8_shift: the shift of match_union8_kernel's 8-bit planes, -1 = chosen from the data (default), 0..3 = fixed."""
    r = load().viso_ctx_set_row8_shift(ctx.h if ctx is not None else None, int(shift))
    if r != 1:
        _err("viso_ctx_set_row8_shift", r)


def set_gn_split(split, ctx=None):
    """viso_ctx_set_gn_split: iterations of a 3-point hypothesis done by the lane-per-hypothesis kernel (0 = default)."""
    r = load().viso_ctx_set_gn_split(ctx.h if ctx is not None else None, int(split))
    if r != 1:
        _err("viso_ctx_set_gn_split", r)


def matcher_kernel_name(ctx=None):
    return load().viso_ctx_matcher_kernel_name(ctx.h if ctx is not None else None).decode()


# Handles that are still open when the interpreter exits are closed HERE, from an atexit hook: that runs before
# the HIP runtime's own teardown, whereas a __del__ during interpreter finalisation can run after it (calling
# hipStreamSynchronize then aborts the process from inside the runtime).  Batches first, then contexts.
_live = weakref.WeakSet()


def _close_all():
    objs = list(_live)
    for o in sorted(objs, key=lambda o: isinstance(o, Context)):
        try:
            o.close()
        except Exception:
            pass


atexit.register(_close_all)


class PinnedArray:
    """numpy view of hipHostMalloc memory (viso_host_alloc) for the *_async uploads."""

    def __init__(self, shape, dtype):
        self.L = load()
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.p = self.L.viso_host_alloc(self.nbytes)
        if not self.p:
            raise VisoError("viso_host_alloc: " + self.L.viso_last_error().decode())
        buf = (C.c_char * self.nbytes).from_address(self.p)
        self.a = np.frombuffer(buf, dtype=dtype).reshape(shape)
        _live.add(self)

    def close(self):
        if self.p:
            self.a = None
            self.L.viso_host_free(self.p)
            self.p = None

    def __del__(self, _finalizing=sys.is_finalizing):   # bound at definition: module globals are None late in shutdown
        if not _finalizing():
            try:
                self.close()
            except Exception:
                pass


# ------------------------------------------------------------ plain family
def match_desc(kp1, kp2, d1, d2, mp):
    """match_desc, reference src/viso.cpp:669-726 -> (M,3) int32 (i1,i2,dist)."""
    L = load()
    kp1, kp2 = _f32(kp1).reshape(-1, 2), _f32(kp2).reshape(-1, 2)
    d1, d2 = _f32(d1), _f32(d2)
    n1, n2 = len(kp1), len(kp2)
    dlen = d1.shape[1] if d1.ndim == 2 else d2.shape[1]
    out = np.empty((max(n1, 1), 3), np.int32)
    n = C.c_int(0)
    r = L.viso_match_desc(ptr(kp1, C.c_float), n1, ptr(kp2, C.c_float), n2, ptr(d1, C.c_float),
                          ptr(d2, C.c_float), dlen, C.byref(mp), ptr(out, C.c_int32), C.byref(n))
    if r != 1:
        _err("viso_match_desc", r)
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
        _err("viso_match_circle", r)
    k = min(n.value, cap)
    return r, circ[:k].copy(), pcl[:k].copy(), n.value


def collect_matches(kp1, kp2, match):
    L = load()
    kp1, kp2 = _f32(kp1).reshape(-1, 2), _f32(kp2).reshape(-1, 2)
    match = _i32(match).reshape(-1, 3)
    x = np.empty((4, len(match)), np.float64)
    r = L.viso_collect_matches(ptr(kp1, C.c_float), len(kp1), ptr(kp2, C.c_float), len(kp2),
                               ptr(match, C.c_int32), len(match), ptr(x, C.c_double))
    if r != 1:
        _err("viso_collect_matches", r)
    return x


def triangulate_rectified(x, param):
    L = load()
    x = _f64(x)
    X = np.empty((3, x.shape[1]), np.float64)
    r = L.viso_triangulate_rectified(ptr(x, C.c_double), x.shape[1], C.byref(param), ptr(X, C.c_double))
    if r != 1:
        _err("viso_triangulate_rectified", r)
    return X


def minimize_reproj(X, obs, tr, param, active):
    L = load()
    X, obs, active = _f64(X), _f64(obs), _i32(active)
    tr = _f64(tr).copy()
    r = L.viso_minimize_reproj(ptr(X, C.c_double), ptr(obs, C.c_double), X.shape[1],
                               ptr(tr, C.c_double), C.byref(param), ptr(active, C.c_int32), len(active))
    if r < 0:
        _err("viso_minimize_reproj", r)
    return r, tr


def get_inliers(X, obs, tr, param):
    L = load()
    X, obs, tr = _f64(X), _f64(obs), _f64(tr)
    m = X.shape[1]
    inl = np.empty(max(m, 1), np.int32)
    n = C.c_int(0)
    rms = C.c_double(0)
    r = L.viso_get_inliers(ptr(X, C.c_double), ptr(obs, C.c_double), m, ptr(tr, C.c_double),
                           C.byref(param), ptr(inl, C.c_int32), C.byref(n), C.byref(rms))
    if r != 1:
        _err("viso_get_inliers", r)
    return inl[:n.value].copy(), rms.value


def support_sizes(X, obs, tr_h, param):
    """Support size of every motion tr_h[k] over (X, obs), through the RANSAC stage's counting kernel."""
    L = load()
    X, obs, tr_h = _f64(X), _f64(obs), _f64(np.atleast_2d(tr_h))
    cnt = np.zeros(max(len(tr_h), 1), np.int32)
    r = L.viso_support_sizes(ptr(X, C.c_double), ptr(obs, C.c_double), X.shape[1], ptr(tr_h, C.c_double), len(tr_h),
                             C.byref(param), ptr(cnt, C.c_int32))
    if r != 1:
        _err("viso_support_sizes", r)
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
        _err("viso_ransac_minimize_reproj", r)
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
    r = L.viso_extract_descriptors(ptr(img, C.c_uint8), img.shape[0], img.shape[1], ptr(kp, C.c_float),
                                   len(kp), radius, ptr(d, C.c_float))
    if r != 1:
        _err("viso_extract_descriptors", r)
    return d


def refine_stereo_subpixel(imgL, imgR, kp1, kp2, match, mode=1):
    """viso_refine_stereo_subpixel: the opt-in sub-pixel refinement of stereo matches (not in the reference;
    include/viso_hip.h).  match: (n, 3) int32 rows (i1, i2, dist) into kp1 / kp2; mode 1 (horizontal) or 2 (both axes).
    Returns (n, 2) float32 refined right-image points (uR', vR')."""
    L = load()
    imgL = np.ascontiguousarray(imgL, dtype=np.uint8)
    imgR = np.ascontiguousarray(imgR, dtype=np.uint8)
    if imgL.shape != imgR.shape or imgL.ndim != 2:
        raise ValueError("refine_stereo_subpixel: the two images must be 2-D and of one size")
    kp1, kp2 = _f32(kp1).reshape(-1, 2), _f32(kp2).reshape(-1, 2)
    match = _i32(match).reshape(-1, 3)
    out = np.empty((max(len(match), 1), 2), np.float32)
    r = L.viso_refine_stereo_subpixel(ptr(imgL, C.c_uint8), ptr(imgR, C.c_uint8), imgL.shape[0], imgL.shape[1],
                                      ptr(kp1, C.c_float), len(kp1), ptr(kp2, C.c_float), len(kp2),
                                      ptr(match, C.c_int32), len(match), int(mode), ptr(out, C.c_float))
    if r != 1:
        _err("viso_refine_stereo_subpixel", r)
    return out[:len(match)].copy()


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
    r = L.viso_rectify_map(ptr(K, C.c_double), ptr(D, C.c_double), ptr(R, C.c_double), ptr(P, C.c_double), rows, cols,
                           ptr(mapx, C.c_float), ptr(mapy, C.c_float))
    if r != 1:
        _err("viso_rectify_map", r)
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
    r = L.viso_rectify_images(ptr(raw, C.c_uint8), n, rr, rc, ptr(mapx, C.c_float), ptr(mapy, C.c_float), rows, cols, int(border),
                              ptr(out, C.c_uint8))
    if r != 1:
        _err("viso_rectify_images", r)
    return out[0].copy() if single else out[:n].copy()


DISP_INVALID = -16   # VISO_DISP_INVALID


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
    imgL = np.ascontiguousarray(imgL, dtype=np.uint8)
    imgR = np.ascontiguousarray(imgR, dtype=np.uint8)
    if imgL.shape != imgR.shape or imgL.ndim != 2:
        raise ValueError("stereo_disparity: the two images must be 2-D and of one size")
    p = disparity_params(**params)
    out = np.empty(imgL.shape, np.int16)
    r = L.viso_stereo_disparity(ptr(imgL, C.c_uint8), ptr(imgR, C.c_uint8), imgL.shape[0], imgL.shape[1], C.byref(p),
                                ptr(out, C.c_int16))
    if r != 1:
        _err("viso_stereo_disparity", r)
    return out


def sgm_params(**params):
    """viso_sgm_params: viso_sgm_params_default with the given fields (num_disp, p1, p2, paths, uniqueness, lr_max_diff) replaced.
    Needs no library: the ranges are checked by the calls that take it (SgmParams.ok restates them)."""
    p = SgmParams(**SGM_DEFAULTS)
    for k, v in params.items():
        if k not in SGM_DEFAULTS:
            raise TypeError(f"sgm_params: unknown parameter {k!r}")
        setattr(p, k, int(v))
    return p


def stereo_sgm(imgL, imgR, **params):
    """viso_stereo_sgm: the dense disparity map of one rectified pair by semi-global matching (opt-in, not in the reference; the
    definition of include/viso_hip.h), on the device.  Returns int16 [rows][cols] in 1/16 px, DISP_INVALID where invalid."""
    L = load()
    imgL = np.ascontiguousarray(imgL, dtype=np.uint8)
    imgR = np.ascontiguousarray(imgR, dtype=np.uint8)
    if imgL.shape != imgR.shape or imgL.ndim != 2:
        raise ValueError("stereo_sgm: the two images must be 2-D and of one size")
    p = sgm_params(**params)
    out = np.empty(imgL.shape, np.int16)
    r = L.viso_stereo_sgm(ptr(imgL, C.c_uint8), ptr(imgR, C.c_uint8), imgL.shape[0], imgL.shape[1], C.byref(p), ptr(out, C.c_int16))
    if r != 1:
        _err("viso_stereo_sgm", r)
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
    p = SpeckleParams(**SPECKLE_DEFAULTS)
    for k, v in params.items():
        if k not in SPECKLE_DEFAULTS:
            raise TypeError(f"speckle_params: unknown parameter {k!r}")
        setattr(p, k, int(v))
    return p


def filter_speckles(d16, **params):
    """viso_filter_speckles: a copy of the int16 map with every 4-connected component of at most max_size pixels (neighbours linked
    when they differ by at most max_diff) set to DISP_INVALID (opt-in, not in the reference; the definition of include/viso_hip.h),
    on the device."""
    d16 = np.asarray(d16)
    if d16.ndim != 2 or d16.dtype != np.int16:
        raise ValueError("filter_speckles: the map must be a 2-D int16 array")
    out = np.array(d16, dtype=np.int16, order="C", copy=True)
    p = speckle_params(**params)
    r = load().viso_filter_speckles(ptr(out, C.c_int16), out.shape[0], out.shape[1], C.byref(p))
    if r != 1:
        _err("viso_filter_speckles", r)
    return out


def speckle_set_workspace_cap(nbytes):
    """viso_speckle_set_workspace_cap: the bytes of label and size words one group of frames may take (0: the default)."""
    load().viso_speckle_set_workspace_cap(int(nbytes))


def speckle_frame_bytes(rows, cols):
    """The workspace of one frame: a label word and a size word per pixel, each plane rounded up to 256 bytes."""
    return 2 * ((rows * cols * 4 + 255) & ~255)


def _pose_arg(where, pose):
    """A pose for the reprojection: None, or a 4 x 4 (or 3 x 4) matrix as contiguous float64 (the first three rows are read)."""
    if pose is None:
        return None, None
    T = np.ascontiguousarray(pose, dtype=np.float64)
    if T.shape not in ((4, 4), (3, 4)):
        raise ValueError(f"{where}: the pose must be a 4 x 4 (or 3 x 4) matrix")
    return T, ptr(T, C.c_double)


def disparity_to_points(d16, param, pose=None, min_disp16=1):
    """viso_disparity_to_points: the int16 map as an organised point image float32 [rows][cols][3] (X, Y, Z in the left camera's
    frame, or transformed by the 4 x 4 pose), three NaNs where the pixel is invalid or its disparity is below min_disp16 (1/16 px).
    param: a Param (f, cu, cv, base).  A point set is `P[np.isfinite(P[..., 2])]`.  With a trajectory:

        poses, valid = hostmath.chain_poses(tr, ok)      # poses[k + 1] places frame valid[k] in frame 0's coordinates
        P = disparity_to_points(batch.disparity(valid[k]), param, pose=poses[k + 1])
    """
    d16 = np.ascontiguousarray(d16)
    if d16.ndim != 2 or d16.dtype != np.int16:
        raise ValueError("disparity_to_points: the map must be a 2-D int16 array")
    T, Tp = _pose_arg("disparity_to_points", pose)
    out = np.empty(d16.shape + (3,), np.float32)
    r = load().viso_disparity_to_points(ptr(d16, C.c_int16), d16.shape[0], d16.shape[1], C.byref(param), Tp, int(min_disp16),
                                        ptr(out, C.c_float))
    if r != 1:
        _err("viso_disparity_to_points", r)
    return out


def map_params(**params):
    """viso_map_params: viso_map_params_default with the given fields (voxel in metres, min_disp16 in 1/16 px, capacity_log2)
    replaced.  Needs no library: the ranges are checked by viso_map_create (MapParams.ok restates them)."""
    p = MapParams(**MAP_DEFAULTS)
    for k, v in params.items():
        if k not in MAP_DEFAULTS:
            raise TypeError(f"map_params: unknown parameter {k!r}")
        setattr(p, k, float(v) if k == "voxel" else int(v))
    return p


def map_entry_centroids(entries, voxel):
    """viso_map_entry_centroid of every entry: float32 [n][3], the mean position of the points fused into each voxel.  Host only."""
    entries = np.ascontiguousarray(entries, dtype=MAP_ENTRY_DTYPE)
    out = np.empty((len(entries), 3), np.float32)
    L = load()
    for i in range(len(entries)):
        r = L.viso_map_entry_centroid(entries[i:i + 1].ctypes.data, float(voxel), ptr(out[i], C.c_float))
        if r != 1:
            _err("viso_map_entry_centroid", r)
    return out


def map_ply_bytes(entries, voxel):
    """The bytes of write_map_ply: a binary little-endian PLY with one vertex per entry, x, y, z the float32 centroid and count a
    uint32, in the entries' order."""
    entries = np.ascontiguousarray(entries, dtype=MAP_ENTRY_DTYPE)
    c = map_entry_centroids(entries, voxel)
    v = np.empty(len(entries), np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("count", "<u4")]))
    v["x"], v["y"], v["z"], v["count"] = c[:, 0], c[:, 1], c[:, 2], entries["count"]
    head = ("ply\nformat binary_little_endian 1.0\ncomment libviso_amd voxel map, voxel %r m\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\nproperty uint count\nend_header\n" % (float(voxel), len(entries)))
    return head.encode("ascii") + v.tobytes()


def write_map_ply(path, entries, voxel):
    """The entries of VoxelMap.entries as a point cloud file (map_ply_bytes)."""
    data = map_ply_bytes(entries, voxel)
    with open(path, "wb") as f:
        f.write(data)


def voxel_box(centre, half_side, voxel):
    """viso_voxel_box_around: (lo, hi), two int32 [3] arrays, the box of the voxels of edge `voxel` that a cube of half-side
    half_side around centre touches: voxel k is inside when lo <= k < hi on every axis (include/viso_hip.h, "Map eviction")."""
    c = np.ascontiguousarray(centre, dtype=np.float64)
    if c.shape != (3,):
        raise ValueError("voxel_box: the centre must have 3 entries")
    b = VoxelBox()
    r = load().viso_voxel_box_around(ptr(c, C.c_double), float(half_side), float(voxel), C.byref(b))
    if r != 1:
        _err("viso_voxel_box_around", r)
    return np.array(b.lo, np.int32), np.array(b.hi, np.int32)


def _box_arg(where, box):
    lo, hi = box
    lo, hi = np.asarray(lo), np.asarray(hi)
    if lo.shape != (3,) or hi.shape != (3,):
        raise ValueError(f"{where}: the box is (lo, hi) with 3 entries each")
    i32 = np.iinfo(np.int32)
    if any(int(v) != v or not i32.min <= int(v) <= i32.max for v in (*lo, *hi)):
        raise ValueError(f"{where}: the box's entries must be int32 values")
    return VoxelBox((C.c_int32 * 3)(*map(int, lo)), (C.c_int32 * 3)(*map(int, hi)))


def merge_entries(*parts):
    """The sum of maps given as entry arrays of one dtype (MAP_ENTRY_DTYPE, TSDF_ENTRY_DTYPE or TSDF_GRAY_ENTRY_DTYPE): every field
    but k summed by key, sorted by key.  Host only; what add_entries does on the device, so the entries that evict handed back
    (an archive) merged with a map's live entries are the map that was never evicted."""
    if not parts:
        raise ValueError("merge_entries: at least one entry array")
    dtype = np.asarray(parts[0]).dtype
    if dtype not in (MAP_ENTRY_DTYPE, TSDF_ENTRY_DTYPE, TSDF_GRAY_ENTRY_DTYPE):
        raise ValueError("merge_entries: not an entry dtype of a map")
    if any(np.asarray(p).dtype != dtype for p in parts):
        raise ValueError("merge_entries: the parts must share one dtype")
    e = np.concatenate([np.asarray(p).reshape(-1) for p in parts])
    k = e["k"].astype(np.int64) + (1 << 20)
    keys, inv = np.unique((k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2], return_inverse=True)
    out = np.zeros(len(keys), dtype)
    for i in range(3):
        out["k"][:, i] = ((keys >> (21 * (2 - i))) & 0x1fffff) - (1 << 20)
    for name in dtype.names[1:]:
        acc = np.zeros(out[name].shape, out[name].dtype)
        np.add.at(acc, inv.reshape(-1), e[name])
        out[name] = acc
    return out


def tsdf_params(**params):
    """viso_tsdf_params: viso_tsdf_params_default with the given fields (voxel in metres, trunc_voxels, min_disp16 in 1/16 px,
    capacity_log2) replaced.  Needs no library: the ranges are checked by viso_tsdf_create (TsdfParams.ok restates them)."""
    p = TsdfParams(**TSDF_DEFAULTS)
    for k, v in params.items():
        if k not in TSDF_DEFAULTS:
            raise TypeError(f"tsdf_params: unknown parameter {k!r}")
        setattr(p, k, float(v) if k == "voxel" else int(v))
    return p


def tsdf_align_params(**params):
    """viso_tsdf_align_params: viso_tsdf_align_params_default with the given fields (min_weight, gate_voxels, max_iters, eps_rot in
    rad, eps_trans in metres, min_pixels) replaced.  Needs no library: the ranges are checked by the calls (TsdfAlignParams.ok
    restates them)."""
    p = TsdfAlignParams(**TSDF_ALIGN_DEFAULTS)
    for k, v in params.items():
        if k not in TSDF_ALIGN_DEFAULTS:
            raise TypeError(f"tsdf_align_params: unknown parameter {k!r}")
        setattr(p, k, float(v) if k in ("gate_voxels", "eps_rot", "eps_trans") else int(v))
    return p


def tsdf_align_gray_params(**params):
    """viso_tsdf_align_gray_params: viso_tsdf_align_gray_params_default with the given fields replaced: those of tsdf_align_params,
    photo_weight (pixels of disparity per gray level) and photo_gate (gray levels).  Needs no library."""
    photo = {k: params.pop(k) for k in tuple(params) if k in TSDF_ALIGN_GRAY_DEFAULTS}
    p = TsdfAlignGrayParams(geo=tsdf_align_params(**params), **TSDF_ALIGN_GRAY_DEFAULTS)
    for k, v in photo.items():
        setattr(p, k, float(v))
    return p


def tsdf_normal_matrix(normal):
    """The 28 sums of a TSDF_NORMAL_DTYPE record as the symmetric int64 [7][7] matrix N, and its counters as a dict."""
    N = np.zeros((7, 7), np.int64)
    iu = np.triu_indices(7)
    N[iu] = normal["n"]
    N.T[iu] = normal["n"]
    return N, {name: int(normal[name]) for name in TSDF_NORMAL_COUNTERS}


def tsdf_normal_gray_matrix(normal):
    """A TSDF_NORMAL_GRAY_DTYPE record as (N, p, counters): the matrix of tsdf_normal_matrix on the sums of both rows, the
    photometric part p of N[6][6], and the nine counters as a dict."""
    N, c = tsdf_normal_matrix(normal)
    c.update({name: int(normal[name]) for name in TSDF_NORMAL_GRAY_COUNTERS})
    return N, int(normal["p"]), c


def tsdf_crossing_points(crossings, voxel):
    """viso_tsdf_crossing_point of every crossing: float32 [n][3], where the averaged signed distance passes through zero between
    the centres of the two voxels.  Host only."""
    crossings = np.ascontiguousarray(crossings, dtype=TSDF_CROSSING_DTYPE)
    out = np.empty((len(crossings), 3), np.float32)
    L = load()
    for i in range(len(crossings)):
        r = L.viso_tsdf_crossing_point(crossings[i:i + 1].ctypes.data, float(voxel), ptr(out[i], C.c_float))
        if r != 1:
            _err("viso_tsdf_crossing_point", r)
    return out


_PLY_XYZW = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("weight", "<u4")]
_PLY_XYZW_HEAD = "property float x\nproperty float y\nproperty float z\nproperty uint weight\n"
_PLY_RGB = [("red", "u1"), ("green", "u1"), ("blue", "u1")]
_PLY_RGB_HEAD = "property uchar red\nproperty uchar green\nproperty uchar blue\n"


def _ply_vertices(where, x, y, z, weight, gray):
    """(the vertex element's property lines, its records): x, y, z, weight and, with gray (uint8, one a vertex), red = green = blue."""
    if gray is not None:
        gray = np.asarray(gray)
        if gray.dtype != np.uint8 or gray.shape != (len(x),):
            raise ValueError(f"{where}: gray must be a uint8 array with one value a vertex")
    v = np.empty(len(x), np.dtype(_PLY_XYZW + (_PLY_RGB if gray is not None else [])))
    v["x"], v["y"], v["z"], v["weight"] = x, y, z, weight
    if gray is not None:
        v["red"] = v["green"] = v["blue"] = gray
    return _PLY_XYZW_HEAD + (_PLY_RGB_HEAD if gray is not None else ""), v


def surface_ply_bytes(crossings, voxel, gray=None):
    """The bytes of write_surface_ply: a binary little-endian PLY with one vertex per crossing, x, y, z the float32 crossing point
    and weight = min(wa, wb) a uint32, in the crossings' order.  gray (uint8 [n], TsdfMap.vertex_gray of the crossings): red, green
    and blue, all equal to it, follow weight."""
    crossings = np.ascontiguousarray(crossings, dtype=TSDF_CROSSING_DTYPE)
    c = tsdf_crossing_points(crossings, voxel)
    props, v = _ply_vertices("surface_ply_bytes", c[:, 0], c[:, 1], c[:, 2], np.minimum(crossings["wa"], crossings["wb"]), gray)
    head = ("ply\nformat binary_little_endian 1.0\ncomment libviso_amd TSDF surface, voxel %r m\nelement vertex %d\n"
            "%send_header\n" % (float(voxel), len(crossings), props))
    return head.encode("ascii") + v.tobytes()


def write_surface_ply(path, crossings, voxel, gray=None):
    """The crossings of TsdfMap.surface as a point cloud file (surface_ply_bytes)."""
    data = surface_ply_bytes(crossings, voxel, gray)
    with open(path, "wb") as f:
        f.write(data)


def mesh_ply_bytes(vertices, triangles, gray=None):
    """The bytes of write_mesh_ply: a binary little-endian PLY; per vertex x, y, z the float32 position and weight a uint32, per
    face a uchar 3 and three int32 vertex indices, both in the order given.  gray (uint8 [n], the third array of
    TsdfMap.mesh(gray=True)): red, green and blue, all equal to it, follow weight."""
    vertices = np.ascontiguousarray(vertices, dtype=TSDF_MESH_VERTEX_DTYPE)
    triangles = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
    if len(triangles) and (int(triangles.max()) >= len(vertices) or len(vertices) > 2 ** 31):
        raise ValueError("mesh_ply_bytes: a triangle refers to a vertex that is not in the list (or is beyond int32)")
    props, v = _ply_vertices("mesh_ply_bytes", vertices["p"][:, 0], vertices["p"][:, 1], vertices["p"][:, 2], vertices["weight"], gray)
    f = np.empty(len(triangles), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    f["n"], f["v"] = 3, triangles
    head = ("ply\nformat binary_little_endian 1.0\ncomment libviso_amd TSDF mesh\nelement vertex %d\n"
            "%selement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(vertices), props, len(triangles)))
    return head.encode("ascii") + v.tobytes() + f.tobytes()


def write_mesh_ply(path, vertices, triangles, gray=None):
    """The mesh of TsdfMap.mesh as a PLY file (mesh_ply_bytes)."""
    data = mesh_ply_bytes(vertices, triangles, gray)
    with open(path, "wb") as f:
        f.write(data)


def disparity_to_float(d16):
    """float32 disparity in pixels (d16 / 16), NaN where invalid."""
    d16 = np.asarray(d16)
    out = d16.astype(np.float32) / np.float32(16)
    out[d16 == DISP_INVALID] = np.nan
    return out


HARRIS_K = float(np.float32(0.04))   # the reference's intended default (float k = .04, src/viso.cpp:915)


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
    r = L.viso_pose_covariance(ptr(X, C.c_double), ptr(obs, C.c_double), m, ptr(tr, C.c_double), ptr(inl, C.c_int32), len(inl),
                               C.byref(param), int(mode), _sigma(sigma), out.ctypes.data)
    if r != 1:
        _err("viso_pose_covariance", r)
    return out


def pose_refine(X, obs, tr, inliers, param, mode=1, sigma=None):
    """viso_pose_refine: the two-frame bundle adjustment of one frame's solve -- X 3 x m, obs 4 x m, tr 6, inliers the final inlier
    list; mode 1 estimates sigma^2, mode 2 takes sigma (pixels).  Returns (record, points): a 0-d MOTION_REFINE_DTYPE array and
    the refined points (3, n) in the order of the used inliers (empty unless status is 1)."""
    L = load()
    X, obs, tr, inl, m = _pose_inputs("pose_refine", X, obs, tr, inliers)
    out = np.zeros((), MOTION_REFINE_DTYPE)
    pts = np.zeros((3, max(len(inl), 1)))
    r = L.viso_pose_refine(ptr(X, C.c_double), ptr(obs, C.c_double), m, ptr(tr, C.c_double), ptr(inl, C.c_int32), len(inl),
                           C.byref(param), int(mode), _sigma(sigma), out.ctypes.data, ptr(pts, C.c_double))
    if r != 1:
        _err("viso_pose_refine", r)
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
    r = L.viso_window_refine(len(frames) + 1, ptr(m, C.c_int), ptr(X, C.c_double), ptr(obs, C.c_double), ptr(left, C.c_int32),
                             ptr(tr, C.c_double), ptr(inl, C.c_int32), ptr(n, C.c_int), C.byref(param), int(mode), _sigma(sigma),
                             out.ctypes.data)
    if r != 1:
        _err("viso_window_refine", r)
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
    r = L.viso_chain_covariances(ptr(tr, C.c_double), ptr(ok, C.c_int32), covs.ctypes.data, n, ptr(out, C.c_double),
                                 ptr(valid, C.c_int32), C.byref(k))
    if r != 1:
        _err("viso_chain_covariances", r)
    return out[:k.value].copy(), valid[:k.value].copy()


def harris_response(img, k=HARRIS_K):
    """cv::cornerHarris(img, R, 3, 5, k, BORDER_DEFAULT) restated (reference src/viso.cpp:930)."""
    L = load()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    r = np.empty(img.shape, np.float32)
    rc = L.viso_harris_response(ptr(img, C.c_uint8), img.shape[0], img.shape[1], k, ptr(r, C.c_float))
    if rc != 1:
        _err("viso_harris_response", rc)
    return r


def detect_harris_binned(img, n_features=1200, nbinx=24, nbiny=5, k=HARRIS_K):
    """HarrisBinnedFeatureDetector::detectImpl, reference src/viso.cpp:926-975."""
    L = load()
    img = np.ascontiguousarray(img, dtype=np.uint8)
    kp = np.empty((max(1, n_features), 2), np.float32)
    resp = np.empty(max(1, n_features), np.float32)
    n = C.c_int(0)
    rc = L.viso_detect_harris_binned(ptr(img, C.c_uint8), img.shape[0], img.shape[1], n_features, nbinx, nbiny, k,
                                     ptr(kp, C.c_float), ptr(resp, C.c_float), C.byref(n))
    if rc != 1:
        _err("viso_detect_harris_binned", rc)
    return kp[:n.value].copy(), resp[:n.value].copy()


# ------------------------------------------------------------ batched family
class Context:
    def __init__(self, device=0, stream=None):
        self.L = load()
        self.h = self.L.viso_ctx_create(device, stream)
        if not self.h:
            raise VisoError("viso_ctx_create: " + self.L.viso_last_error().decode())
        self._batches = weakref.WeakSet()   # closed with the context: a batch destroyed after its context uses freed streams
        _live.add(self)

    def synchronize(self):
        r = self.L.viso_ctx_synchronize(self.h)
        if r != 1:
            _err("viso_ctx_synchronize", r)

    def close(self):
        if self.h:
            # its batches first, whatever order the caller (or the garbage collector, after an exception skipped the
            # caller's close() calls) takes: viso_batch_destroy on a destroyed context aborts inside the HIP runtime
            for b in list(self._batches):
                try:
                    b.close()
                except Exception:
                    pass
            h, self.h = self.h, None
            r = self.L.viso_ctx_destroy(h)
            if r != 1:
                _err("viso_ctx_destroy", r)

    def __del__(self, _finalizing=sys.is_finalizing):   # bound at definition: module globals are None late in shutdown
        if _finalizing():   # the atexit hook has closed everything that was still open
            return
        try:
            self.close()
        except Exception:
            pass


class _TableMap:
    """What VoxelMap and TsdfMap share: a handle of one of the two kinds of hash tables of voxels (csrc/voxel_host.h).  A subclass
    sets _prefix (the C functions are _prefix + name), _Params and _params (the parameter struct and its factory), _ENTRY_DTYPE and
    _Counters."""

    def __init__(self, ctx=None, params=None, **kw):
        name = type(self).__name__
        self.L = load()
        if isinstance(params, self._Params):
            if kw:
                raise TypeError(f"{name}: keyword fields cannot be combined with a {self._Params.__name__}")
        else:
            params = type(self)._params(**dict(params or {}, **kw))
        self.ctx, self._p, self.voxel = ctx, params, float(params.voxel)
        h = C.c_void_p()
        r = self._c("create")(ctx.h if ctx is not None else None, C.byref(params), C.byref(h))
        self.h = h.value if r == 1 else None
        if r != 1:
            _err(self._prefix + "create", r)
        _live.add(self)

    def _c(self, name):
        return getattr(self.L, self._prefix + name)

    def _chk(self, where, r):
        if r != 1:
            _err(where, r)

    def fuse(self, d16, param, pose=None):
        """viso_map_fuse / viso_tsdf_fuse: one host int16 map with the calibration of param (f, cu, cv, base) and an optional 4 x 4
        pose."""
        where = type(self).__name__ + ".fuse"
        d16 = np.ascontiguousarray(d16)
        if d16.ndim != 2 or d16.dtype != np.int16:
            raise ValueError(f"{where}: the map must be a 2-D int16 array")
        if pose is not None and np.shape(pose) != (4, 4):
            raise ValueError(f"{where}: the pose must be a 4 x 4 matrix")
        T, Tp = _pose_arg(where, pose)
        self._chk(self._prefix + "fuse", self._c("fuse")(self.h, ptr(d16, C.c_int16), d16.shape[0], d16.shape[1], C.byref(param), Tp))

    def add_entries(self, entries):
        """viso_map_add_entries / viso_tsdf_add_entries: the entries of another map with the same voxel (a TSDF map: and truncation),
        or of a saved one, added to this one."""
        entries = np.ascontiguousarray(entries, dtype=self._ENTRY_DTYPE)
        self._chk(self._prefix + "add_entries", self._c("add_entries")(self.h, entries.ctypes.data, len(entries)))

    def _count(self, count_name, threshold):
        n = C.c_size_t()
        self._chk(self._prefix + count_name, self._c(count_name)(self.h, int(threshold), C.byref(n)))
        return n

    def _list(self, count_name, get_name, dtype, threshold):
        n = self._count(count_name, threshold)
        out = np.zeros(n.value, dtype)
        self._chk(self._prefix + get_name, self._c(get_name)(self.h, int(threshold), out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value]

    def _evict_dtype(self):
        return self._ENTRY_DTYPE

    def evict_count(self, box):
        """viso_map_evict_count / viso_tsdf_evict_count: the number of voxels outside box = (lo, hi); reads only."""
        where = type(self).__name__ + ".evict_count"
        n = C.c_size_t()
        self._chk(self._prefix + "evict_count", self._c("evict_count")(self.h, C.byref(_box_arg(where, box)), C.byref(n)))
        return n.value

    def evict(self, box, discard=False):
        """viso_map_evict / viso_tsdf_evict / viso_tsdf_evict_gray: every voxel outside box = (lo, hi) (voxel_box makes one around
        a point) leaves the map, on the device, and its slot is free again.  Returns the evicted voxels as an array of the map's
        own entry dtype (a gray map's: TSDF_GRAY_ENTRY_DTYPE), sorted by key; merge_entries of them and of what the map holds
        later is the map that was never evicted.  discard=True: they are dropped on the device, and their number comes back."""
        where = type(self).__name__ + ".evict"
        b = _box_arg(where, box)
        dtype = self._evict_dtype()
        name = "evict_gray" if dtype == TSDF_GRAY_ENTRY_DTYPE else "evict"
        n = C.c_size_t()
        if discard:
            self._chk(self._prefix + name, self._c(name)(self.h, C.byref(b), None, 0, C.byref(n)))
            return n.value
        self._chk(self._prefix + "evict_count", self._c("evict_count")(self.h, C.byref(b), C.byref(n)))
        out = np.zeros(n.value, dtype)
        self._chk(self._prefix + name, self._c(name)(self.h, C.byref(b), out.ctypes.data, len(out), C.byref(n)))
        return out[:n.value]

    def stats(self):
        """viso_map_stats / viso_tsdf_stats as a dict of the counters' fields."""
        c = self._Counters()
        self._chk(self._prefix + "stats", self._c("stats")(self.h, C.byref(c)))
        return {name: int(getattr(c, name)) for name, _ in self._Counters._fields_}

    def clear(self):
        self._chk(self._prefix + "clear", self._c("clear")(self.h))

    def close(self):
        if self.h:
            h, self.h = self.h, None
            r = self._c("destroy")(h)
            if r != 1:
                _err(self._prefix + "destroy", r)

    def __del__(self, _finalizing=sys.is_finalizing):   # bound at definition: module globals are None late in shutdown
        if _finalizing():   # the atexit hook has closed everything that was still open
            return
        try:
            self.close()
        except Exception:
            pass


class VoxelMap(_TableMap):
    """viso_map: a persistent voxel map on the device that dense disparity maps and their poses are fused into (opt-in, not in the
    reference; the definition of include/viso_hip.h).  ctx: a Context, or None for the default one.  With a trajectory:

        poses, valid = hostmath.chain_poses(tr, ok)      # poses[k + 1] places frame valid[k] in frame 0's coordinates
        vmap = VoxelMap(ctx, voxel=0.2)
        for k, t in enumerate(valid):
            batch.fuse_disparities(vmap, poses[k + 1][None], t0=t, t1=t + 1)
        write_map_ply("scene.ply", vmap.entries(min_count=2), vmap.voxel)
    """
    _prefix, _Params, _params, _ENTRY_DTYPE, _Counters = "viso_map_", MapParams, map_params, MAP_ENTRY_DTYPE, MapCounters

    def count(self, min_count=1):
        return self._count("count", min_count).value

    def entries(self, min_count=1):
        """viso_map_get: the voxels with at least min_count points as a MAP_ENTRY_DTYPE array (k, count, sum), sorted by key."""
        return self._list("count", "get", MAP_ENTRY_DTYPE, min_count)

    def centroids(self, min_count=1):
        """float32 [n][3]: the centroids of entries(min_count), in their order."""
        return map_entry_centroids(self.entries(min_count), self.voxel)


class TsdfMap(_TableMap):
    """viso_tsdf: a persistent map of truncated signed distances on the device that dense disparity maps and their poses are fused
    into, read back as voxels or as the points where the averaged distance changes sign (opt-in, not in the reference; the
    definition of include/viso_hip.h).  ctx: a Context, or None for the default one.  With a trajectory:

        poses, valid = hostmath.chain_poses(tr, ok)      # poses[k + 1] places frame valid[k] in frame 0's coordinates
        tsdf = TsdfMap(ctx, voxel=0.2)
        for k, t in enumerate(valid):
            batch.fuse_tsdf(tsdf, poses[k + 1][None], t0=t, t1=t + 1)
        write_surface_ply("surface.ply", tsdf.surface(min_weight=2), tsdf.voxel)
        write_mesh_ply("mesh.ply", *tsdf.mesh(min_weight=2))

    gray=True: a gray map (include/viso_hip.h, "TSDF intensity"), which also sums the 8-bit intensity of the left images per voxel:
    fuse then takes the image with the map (Batch.fuse_tsdf reads the resident ones), entries(gray=True), mesh(gray=True) and
    render(gray=True) give the intensity with the geometry, and write_mesh_ply("mesh.ply", *tsdf.mesh(2, gray=True)) writes it.
    """
    _prefix, _Params, _params, _ENTRY_DTYPE, _Counters = "viso_tsdf_", TsdfParams, tsdf_params, TSDF_ENTRY_DTYPE, TsdfCounters

    def __init__(self, ctx=None, params=None, gray=False, **kw):
        self.gray = bool(gray)
        super().__init__(ctx, params, **kw)
        self.trunc_voxels = int(self._p.trunc_voxels)

    def _c(self, name):
        return super()._c("create_gray" if name == "create" and self.gray else name)

    def fuse(self, d16, param, pose=None, image=None):
        """viso_tsdf_fuse, or for a gray map viso_tsdf_fuse_gray: one host int16 map with the calibration of param (f, cu, cv, base)
        and an optional 4 x 4 pose.  image: the left image the map was computed from, a 2-D uint8 array of the map's shape, for a
        gray map, and only for one."""
        if (image is not None) != self.gray:
            raise ValueError("TsdfMap.fuse: a gray map is fused with an image, a plain one without")
        if not self.gray:
            return super().fuse(d16, param, pose)
        d16, image = np.ascontiguousarray(d16), np.ascontiguousarray(image)
        if d16.ndim != 2 or d16.dtype != np.int16:
            raise ValueError("TsdfMap.fuse: the map must be a 2-D int16 array")
        if image.dtype != np.uint8 or image.shape != d16.shape:
            raise ValueError("TsdfMap.fuse: the image must be a 2-D uint8 array of the map's shape")
        if pose is not None and np.shape(pose) != (4, 4):
            raise ValueError("TsdfMap.fuse: the pose must be a 4 x 4 matrix")
        T, Tp = _pose_arg("TsdfMap.fuse", pose)
        self._chk("viso_tsdf_fuse_gray", self.L.viso_tsdf_fuse_gray(self.h, ptr(d16, C.c_int16), ptr(image, C.c_uint8), d16.shape[0],
                                                                    d16.shape[1], C.byref(param), Tp))

    def add_entries(self, entries):
        """viso_tsdf_add_entries, or for a TSDF_GRAY_ENTRY_DTYPE array viso_tsdf_add_gray_entries: the entries of another map of
        the same kind, voxel and truncation, or of a saved one, added to this one."""
        if getattr(entries, "dtype", None) != TSDF_GRAY_ENTRY_DTYPE:
            return super().add_entries(entries)
        entries = np.ascontiguousarray(entries)
        self._chk("viso_tsdf_add_gray_entries", self.L.viso_tsdf_add_gray_entries(self.h, entries.ctypes.data, len(entries)))

    def _evict_dtype(self):
        return TSDF_GRAY_ENTRY_DTYPE if self.gray else TSDF_ENTRY_DTYPE

    def entries(self, min_weight=1, gray=False):
        """viso_tsdf_get: the voxels with at least min_weight updates as a TSDF_ENTRY_DTYPE array (k, weight, sum), sorted by key.
        gray=True (a gray map): viso_tsdf_get_gray, a TSDF_GRAY_ENTRY_DTYPE array (k, weight, sum, gray)."""
        if gray:
            return self._list("count", "get_gray", TSDF_GRAY_ENTRY_DTYPE, min_weight)
        return self._list("count", "get", TSDF_ENTRY_DTYPE, min_weight)

    def vertex_gray(self, vertices, missing=False):
        """viso_tsdf_vertex_gray: uint8 [n], the intensity of every vertex of mesh() (a TSDF_MESH_VERTEX_DTYPE array, of which k and
        dir are read) or of every crossing of surface() (a TSDF_CROSSING_DTYPE array: dir = 1 << axis).  0 where an end of the edge
        is not in the table or the ends do not differ in sign; missing=True: a tuple with their number."""
        if getattr(vertices, "dtype", None) == TSDF_CROSSING_DTYPE:
            c = vertices
            vertices = np.zeros(len(c), TSDF_MESH_VERTEX_DTYPE)
            vertices["k"], vertices["dir"] = c["k"], np.left_shift(1, c["axis"])
        vertices = np.ascontiguousarray(vertices, dtype=TSDF_MESH_VERTEX_DTYPE)
        g, n_missing = np.zeros(len(vertices), np.uint8), C.c_size_t()
        self._chk("viso_tsdf_vertex_gray", self.L.viso_tsdf_vertex_gray(self.h, vertices.ctypes.data, len(vertices), ptr(g, C.c_uint8),
                                                                        C.byref(n_missing)))
        return (g, n_missing.value) if missing else g

    def surface(self, min_weight=1):
        """viso_tsdf_surface: the sign changes between neighbouring voxels of at least min_weight updates as a TSDF_CROSSING_DTYPE
        array (k, axis, wa, wb, sa, sb), sorted by (key, axis)."""
        return self._list("surface_count", "surface", TSDF_CROSSING_DTYPE, min_weight)

    def surface_points(self, min_weight=1):
        """float32 [n][3]: the crossing points of surface(min_weight), in their order."""
        return tsdf_crossing_points(self.surface(min_weight), self.voxel)

    def mesh(self, min_weight=1, gray=False):
        """viso_tsdf_mesh: the surface as triangles by marching tetrahedra over the voxels of at least min_weight updates.  Returns
        (vertices, triangles): a TSDF_MESH_VERTEX_DTYPE array (k, dir, p, weight) sorted by (key, dir), and uint32 [n][3] indices
        into it sorted by (cell, tetrahedron, index), the normals towards the side the surface was seen from.  gray=True (a gray
        map): (vertices, triangles, g), g = vertex_gray(vertices)."""
        nv, nt = C.c_size_t(), C.c_size_t()
        self._chk("viso_tsdf_mesh_count", self.L.viso_tsdf_mesh_count(self.h, int(min_weight), C.byref(nv), C.byref(nt)))
        v, tri = np.zeros(nv.value, TSDF_MESH_VERTEX_DTYPE), np.zeros((nt.value, 3), np.uint32)
        self._chk("viso_tsdf_mesh", self.L.viso_tsdf_mesh(self.h, int(min_weight), v.ctypes.data, len(v), tri.ctypes.data, len(tri),
                                                          C.byref(nv), C.byref(nt)))
        v, tri = v[:nv.value], tri[:nt.value]
        return (v, tri, self.vertex_gray(v)) if gray else (v, tri)

    def _align_args(self, where, d16, pose):
        d16 = np.ascontiguousarray(d16)
        if d16.ndim != 2 or d16.dtype != np.int16:
            raise ValueError(f"{where}: the map must be a 2-D int16 array")
        if pose is not None and np.shape(pose) != (4, 4):
            raise ValueError(f"{where}: the pose must be a 4 x 4 matrix")
        return (d16,) + _pose_arg(where, pose)

    def _align_image(self, where, image, d16):
        """The image of a photometric call: uint8, the map's shape, and only with a gray map."""
        if not self.gray:
            raise ValueError(f"{where}: an image goes with a gray map (TsdfMap(gray=True))")
        image = np.ascontiguousarray(image)
        if image.dtype != np.uint8 or image.shape != d16.shape:
            raise ValueError(f"{where}: the image must be a uint8 array of the map's shape")
        return image

    def linearize(self, d16, param, pose=None, image=None, **params):
        """viso_tsdf_linearize: the integer normal equations of the frame-to-model alignment (include/viso_hip.h, "TSDF align") of
        one host int16 map at the 4 x 4 camera-to-world pose (None: the identity).  Returns (N, counters): the symmetric int64
        [7][7] matrix of the six entries of the rows and the residual, and a dict of n_points, n_used, n_missing, n_gated,
        n_clipped, n_out_of_range.  params: the fields of tsdf_align_params.  Reads the map only.
        image (uint8, the map's shape; a gray map): viso_tsdf_linearize_gray ("TSDF photometric align"), the left image the map was
        computed from; params then also takes photo_weight and photo_gate, and the result is (N, p, counters): N with the products
        of both rows, p the photometric part of N[6][6], and n_photo_used, n_photo_gated, n_photo_clipped among the counters."""
        d16, T, Tp = self._align_args("TsdfMap.linearize", d16, pose)
        if image is not None:
            image = self._align_image("TsdfMap.linearize", image, d16)
            p, out = tsdf_align_gray_params(**params), np.zeros(1, TSDF_NORMAL_GRAY_DTYPE)
            self._chk("viso_tsdf_linearize_gray", self.L.viso_tsdf_linearize_gray(self.h, C.byref(p), ptr(d16, C.c_int16), ptr(image, C.c_uint8),
                                                                                  d16.shape[0], d16.shape[1], C.byref(param), Tp, out.ctypes.data))
            return tsdf_normal_gray_matrix(out[0])
        p, out = tsdf_align_params(**params), np.zeros(1, TSDF_NORMAL_DTYPE)
        self._chk("viso_tsdf_linearize", self.L.viso_tsdf_linearize(self.h, C.byref(p), ptr(d16, C.c_int16), d16.shape[0], d16.shape[1],
                                                                    C.byref(param), Tp, out.ctypes.data))
        return tsdf_normal_matrix(out[0])

    def align(self, d16, param, pose=None, trace=False, image=None, **params):
        """viso_tsdf_align: the pose at which the points of one host int16 map lie on the map's surface, from the guess `pose` (4 x 4,
        camera to world; None: the identity).  Returns a TSDF_ALIGNMENT_DTYPE record (pose, cov of (v, omega), cost in pixels of
        disparity, n_used, iters, status: 1 converged, 2 max_iters reached, < 0 failed and pose is the guess).  trace=True: a tuple
        with the TSDF_ALIGN_STEP_DTYPE array of the linearises (pose, normal), the last one included.  params: the fields of
        tsdf_align_params.  Reads the map only.
        image (uint8, the map's shape; a gray map): viso_tsdf_align_gray ("TSDF photometric align"), every used pixel also pulls the
        model's intensity to its own; params then also takes photo_weight and photo_gate, the record is a TSDF_ALIGNMENT_GRAY_DTYPE
        one (the same fields, then cost_geo in pixels, cost_photo in gray levels and n_photo_used) and the trace a
        TSDF_ALIGN_GRAY_STEP_DTYPE array."""
        d16, T, Tp = self._align_args("TsdfMap.align", d16, pose)
        if image is not None:
            image = self._align_image("TsdfMap.align", image, d16)
            p, rec = tsdf_align_gray_params(**params), np.zeros(1, TSDF_ALIGNMENT_GRAY_DTYPE)
            steps = np.zeros(p.geo.max_iters + 1 if trace and 1 <= p.geo.max_iters <= 50 else 0, TSDF_ALIGN_GRAY_STEP_DTYPE)
            self._chk("viso_tsdf_align_gray", self.L.viso_tsdf_align_gray(self.h, C.byref(p), ptr(d16, C.c_int16), ptr(image, C.c_uint8), d16.shape[0],
                                                                          d16.shape[1], C.byref(param), Tp, rec.ctypes.data,
                                                                          steps.ctypes.data if len(steps) else None, len(steps)))
            return (rec[0], steps[steps["pose"][:, 3, 3] == 1.0]) if trace else rec[0]
        p, rec = tsdf_align_params(**params), np.zeros(1, TSDF_ALIGNMENT_DTYPE)
        steps = np.zeros(p.max_iters + 1 if trace and 1 <= p.max_iters <= 50 else 0, TSDF_ALIGN_STEP_DTYPE)
        self._chk("viso_tsdf_align", self.L.viso_tsdf_align(self.h, C.byref(p), ptr(d16, C.c_int16), d16.shape[0], d16.shape[1], C.byref(param),
                                                            Tp, rec.ctypes.data, steps.ctypes.data if len(steps) else None, len(steps)))
        if not trace:
            return rec[0]
        return rec[0], steps[steps["pose"][:, 3, 3] == 1.0]   # a written step's pose ends in 0 0 0 1

    def render(self, param, shape, poses=None, max_depth=40.0, min_weight=2, weights=False, gray=False):
        """viso_tsdf_render: what a camera with the calibration of param (f, cu, cv, base) would see of the map, by ray casting: an
        int16 disparity map in 1/16 px of shape (rows, cols), VISO_DISP_INVALID where the ray meets no surface from its front within
        max_depth metres.  poses: None (no transform), one 4 x 4 camera-to-world matrix, as fuse takes it (returns [rows][cols]), or
        [n][4][4] (returns [n][rows][cols], the views of one call).  min_weight: only voxels with at least this many updates.
        weights=True: a tuple with the uint32 array of the same shape, the smaller weight of the two voxels of a hit (0: none).
        gray=True (a gray map): viso_tsdf_render_gray, the tuple ends with the uint8 array of the same shape, the intensity of the
        hit (0: none)."""
        rows, cols = (int(v) for v in shape)
        T = None
        if poses is not None:
            T = np.ascontiguousarray(poses, dtype=np.float64)
            if T.shape[-2:] != (4, 4) or T.ndim not in (2, 3) or T.size == 0:
                raise ValueError("TsdfMap.render: poses must be None, a 4 x 4 matrix or [n][4][4]")
        n = 1 if T is None or T.ndim == 2 else len(T)
        if rows < 1 or cols < 1:
            raise ValueError("TsdfMap.render: shape must be (rows, cols), both >= 1")
        d = np.empty((n, rows, cols), np.int16)
        w = np.empty((n, rows, cols), np.uint32) if weights else None
        g = np.empty((n, rows, cols), np.uint8) if gray else None
        args = (self.h, int(min_weight), C.byref(param), rows, cols, float(max_depth), ptr(T, C.c_double) if T is not None else None, n,
                ptr(d, C.c_int16), ptr(w, C.c_uint32) if weights else None)
        if gray:
            self._chk("viso_tsdf_render_gray", self.L.viso_tsdf_render_gray(*args, ptr(g, C.c_uint8)))
        else:
            self._chk("viso_tsdf_render", self.L.viso_tsdf_render(*args))
        if T is None or T.ndim == 2:
            d, w, g = d[0], (w[0] if weights else None), (g[0] if gray else None)
        out = (d,) + ((w,) if weights else ()) + ((g,) if gray else ())
        return out if len(out) > 1 else d


class Batch:
    """viso_batch: n_frames stereo frames resident in HBM (include/viso_hip.h)."""

    def __init__(self, ctx, n_frames, cap, dlen=DESC_LEN):
        self.ctx, self.L = ctx, ctx.L
        self.nf, self.cap, self.dlen = n_frames, cap, dlen
        self.h = self.L.viso_batch_create(ctx.h, n_frames, cap, dlen)
        if not self.h:
            raise VisoError("viso_batch_create: " + self.L.viso_last_error().decode())
        ctx._batches.add(self)
        _live.add(self)

    def _chk(self, where, r):
        if r != 1:
            _err(where, r)

    def upload(self, kp, desc, n, f0=0):
        kp, desc, n = _f32(kp), _f32(desc), _i32(n)
        nf = kp.shape[0]
        assert kp.shape == (nf, 2, self.cap, 2) and desc.shape == (nf, 2, self.cap, self.dlen)
        self._chk("viso_batch_upload", self.L.viso_batch_upload(self.h, f0, nf, ptr(kp, C.c_float),
                                                                 ptr(desc, C.c_float), ptr(n, C.c_int32)))

    def upload_async(self, kp, desc, n, f0=0):
        """Enqueue the copies on the context's stream; kp/desc should be PinnedArray views and must stay untouched
        until the stream has passed them."""
        assert kp.dtype == np.float32 and desc.dtype == np.float32 and kp.flags.c_contiguous and desc.flags.c_contiguous
        n = _i32(n)
        nf = kp.shape[0]
        self._chk("viso_batch_upload_async", self.L.viso_batch_upload_async(self.h, f0, nf, ptr(kp, C.c_float),
                                                                             ptr(desc, C.c_float), ptr(n, C.c_int32)))

    def upload_i16(self, kp, desc16, n, f0=0, asynchronous=False):
        """Descriptors as int16 [nf][2][cap][dlen] (the lossless encoding of the Sobel windows; half the bytes).
        asynchronous=True: enqueued on the context's stream; kp / desc16 should be PinnedArray views."""
        kp, n = _f32(kp), _i32(n)
        assert desc16.dtype == np.int16 and desc16.flags.c_contiguous
        nf = kp.shape[0]
        assert kp.shape == (nf, 2, self.cap, 2) and desc16.shape == (nf, 2, self.cap, self.dlen)
        fn = self.L.viso_batch_upload_i16_async if asynchronous else self.L.viso_batch_upload_i16
        self._chk("viso_batch_upload_i16", fn(self.h, f0, nf, ptr(kp, C.c_float), ptr(desc16, C.c_int16), ptr(n, C.c_int32)))

    def upload_images_async(self, images, kp, n, f0=0):
        assert images.dtype == np.uint8 and images.flags.c_contiguous and kp.dtype == np.float32 and kp.flags.c_contiguous
        n = _i32(n)
        nf, _, rows, cols = images.shape
        self._chk("viso_batch_upload_images_async", self.L.viso_batch_upload_images_async(
            self.h, f0, nf, ptr(images, C.c_uint8), rows, cols, ptr(kp, C.c_float), ptr(n, C.c_int32)))

    def upload_images(self, images, kp, n, f0=0):
        """Image-in mode: uint8 images [nf][2][rows][cols] + keypoints (descriptors are extracted on the device)."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        kp, n = _f32(kp), _i32(n)
        nf, _, rows, cols = images.shape
        assert kp.shape == (nf, 2, self.cap, 2)
        self._chk("viso_batch_upload_images", self.L.viso_batch_upload_images(
            self.h, f0, nf, ptr(images, C.c_uint8), rows, cols, ptr(kp, C.c_float), ptr(n, C.c_int32)))

    def upload_images_only(self, images, f0=0):
        """Images without keypoints: follow with detect()."""
        images = np.ascontiguousarray(images, dtype=np.uint8)
        nf, _, rows, cols = images.shape
        self._chk("viso_batch_upload_images", self.L.viso_batch_upload_images(
            self.h, f0, nf, ptr(images, C.c_uint8), rows, cols, None, None))

    def detect(self, n_features=1200, nbinx=24, nbiny=5, k=HARRIS_K):
        self._chk("viso_batch_detect", self.L.viso_batch_detect(self.h, n_features, nbinx, nbiny, k))

    def keypoints(self, t, side):
        kp = np.empty((self.cap, 2), np.float32)
        n = C.c_int(0)
        self._chk("viso_batch_get_keypoints", self.L.viso_batch_get_keypoints(self.h, t, side, ptr(kp, C.c_float), C.byref(n)))
        return kp[:n.value].copy()

    def run_images(self, matcher_only=False):
        self._chk("viso_batch_run_images", self.L.viso_batch_run_images(self.h, int(matcher_only)))

    def set_subpixel(self, mode):
        """viso_batch_set_subpixel: 0 = off (default), 1 = refine the stereo matches' uR, 2 = uR and vR (image-in runs only)."""
        self._chk("viso_batch_set_subpixel", self.L.viso_batch_set_subpixel(self.h, int(mode)))

    def subpixel(self, t):
        """(n, 2) float32 refined (uR', vR') of frame t's stereo rows from the last run, in the order of matches(0, t)."""
        out = np.empty((self.cap, 2), np.float32)
        n = C.c_int(0)
        self._chk("viso_batch_get_subpixel", self.L.viso_batch_get_subpixel(self.h, t, ptr(out, C.c_float), C.byref(n)))
        return out[:n.value].copy()

    def set_rectify(self, raw_shape, out_shape=None, left=None, right=None, border=0):
        """viso_batch_set_rectify: from the next image upload on, uploads take raw images of raw_shape (rows, cols) and the device
        rectifies them to out_shape with the maps left = (mapx, mapy) and right = (mapx, mapy) (rectify_map).  set_rectify(None)
        turns it off."""
        if raw_shape is None:
            self._chk("viso_batch_set_rectify", self.L.viso_batch_set_rectify(self.h, 0, 0, 0, 0, None, None, None, None, 0))
            return
        if left is None or right is None or out_shape is None:
            raise ValueError("set_rectify: out_shape and both maps are needed (or raw_shape=None to turn it off)")
        rows, cols = (int(v) for v in out_shape)
        lx, ly = _map_pair(left[0], left[1], (rows, cols))
        rx, ry = _map_pair(right[0], right[1], (rows, cols))
        rr, rc = (int(v) for v in raw_shape)
        self._chk("viso_batch_set_rectify", self.L.viso_batch_set_rectify(
            self.h, rr, rc, rows, cols, ptr(lx, C.c_float), ptr(ly, C.c_float), ptr(rx, C.c_float), ptr(ry, C.c_float), int(border)))

    def image_shape(self):
        """(rows, cols) of the device images (viso_batch_get_image_geometry); (0, 0) before any image upload."""
        r, c = C.c_int(0), C.c_int(0)
        self._chk("viso_batch_get_image_geometry", self.L.viso_batch_get_image_geometry(self.h, C.byref(r), C.byref(c)))
        return r.value, c.value

    def image(self, t, side):
        """The device image of frame t, side (uint8, rectified when rectification was on at its upload)."""
        shape = self.image_shape()   # the library's geometry, not a copy of it here: the buffer always fits what is copied
        if shape == (0, 0):
            raise VisoError("Batch.image: no images uploaded")
        out = np.empty(shape, np.uint8)
        self._chk("viso_batch_get_image", self.L.viso_batch_get_image(self.h, int(t), int(side), ptr(out, C.c_uint8)))
        return out

    def set_disparity(self, params=None, **kw):
        """viso_batch_set_disparity: dense disparity of every frame's resident pair in the next image-in runs (run_images, also
        matcher_only) and in run_disparity.  params: a DisparityParams, a dict of its fields, or keyword fields (defaults for the
        rest); set_disparity(None) turns it off (the default)."""
        if params is None and not kw:
            self._chk("viso_batch_set_disparity", self.L.viso_batch_set_disparity(self.h, None))
            return
        if isinstance(params, DisparityParams):
            if kw:
                raise TypeError("set_disparity: keyword fields cannot be combined with a DisparityParams")
        else:
            params = disparity_params(**dict(params or {}, **kw))
        self._chk("viso_batch_set_disparity", self.L.viso_batch_set_disparity(self.h, C.byref(params)))

    def set_sgm(self, params=None, **kw):
        """viso_batch_set_sgm: the batch's dense maps by semi-global matching in the next image-in runs and in run_disparity
        (run_disparity / disparity / disparities serve them).  params: an SgmParams, a dict of its fields, or keyword fields
        (defaults for the rest); set_sgm(None) turns it off (the default).  One method at a time: refused while set_disparity is
        on."""
        if params is None and not kw:
            self._chk("viso_batch_set_sgm", self.L.viso_batch_set_sgm(self.h, None))
            return
        if isinstance(params, SgmParams):
            if kw:
                raise TypeError("set_sgm: keyword fields cannot be combined with an SgmParams")
        else:
            params = sgm_params(**dict(params or {}, **kw))
        self._chk("viso_batch_set_sgm", self.L.viso_batch_set_sgm(self.h, C.byref(params)))

    def set_speckle(self, params=None, **kw):
        """viso_batch_set_speckle: the speckle filter over the batch's maps, right behind whichever method is on (set_disparity or
        set_sgm), in the next image-in runs and in run_disparity; disparity / disparities serve the filtered maps.  params: a
        SpeckleParams, a dict of its fields, or keyword fields (defaults for the rest); set_speckle(None) turns it off (the
        default).  With no method on it does nothing."""
        if params is None and not kw:
            self._chk("viso_batch_set_speckle", self.L.viso_batch_set_speckle(self.h, None))
            return
        if isinstance(params, SpeckleParams):
            if kw:
                raise TypeError("set_speckle: keyword fields cannot be combined with a SpeckleParams")
        else:
            params = speckle_params(**dict(params or {}, **kw))
        self._chk("viso_batch_set_speckle", self.L.viso_batch_set_speckle(self.h, C.byref(params)))

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
        self._chk("viso_batch_get_disparity_points",
                  self.L.viso_batch_get_disparity_points(self.h, int(t), Tp, int(min_disp16), ptr(out, C.c_float)))
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
        self._chk("viso_batch_fuse_disparities", self.L.viso_batch_fuse_disparities(self.h, vmap.h, int(t0), t1, ptr(T, C.c_double)))

    def fuse_tsdf(self, tsdf, poses, t0=0, t1=None):
        """viso_batch_fuse_tsdf: the resident maps of frames t0 .. t1-1 (t1 None: to the last frame) fused into the TsdfMap on the
        device, frame t0 + i with the 4 x 4 pose poses[i]; no map is copied to the host.  The map must be on this batch's context."""
        t1, T = self._range_poses("Batch.fuse_tsdf", poses, t0, t1)
        self._chk("viso_batch_fuse_tsdf", self.L.viso_batch_fuse_tsdf(self.h, tsdf.h, int(t0), t1, ptr(T, C.c_double)))

    def align_tsdf(self, tsdf, poses, t0=0, t1=None, photo=False, **params):
        """viso_batch_align_tsdf: the resident maps of frames t0 .. t1-1 (t1 None: to the last frame) aligned against the TsdfMap, each
        on its own from the 4 x 4 guess poses[i]; no map is copied to the host.  Returns a TSDF_ALIGNMENT_DTYPE array [t1 - t0], each
        what TsdfMap.align gives for that map and guess.  params: the fields of tsdf_align_params.  The map must be on this batch's
        context.
        photo=True (a gray map): viso_batch_align_tsdf_gray, with frame t's resident left image; params also takes photo_weight and
        photo_gate, and the records are TSDF_ALIGNMENT_GRAY_DTYPE ones: cost_geo, cost_photo and n_photo_used follow the fields."""
        t1, T = self._range_poses("Batch.align_tsdf", poses, t0, t1)
        if photo:
            p, rec = tsdf_align_gray_params(**params), np.zeros(len(T), TSDF_ALIGNMENT_GRAY_DTYPE)
            self._chk("viso_batch_align_tsdf_gray", self.L.viso_batch_align_tsdf_gray(self.h, tsdf.h, int(t0), t1, ptr(T, C.c_double), C.byref(p),
                                                                                      rec.ctypes.data))
            return rec
        p, rec = tsdf_align_params(**params), np.zeros(len(T), TSDF_ALIGNMENT_DTYPE)
        self._chk("viso_batch_align_tsdf", self.L.viso_batch_align_tsdf(self.h, tsdf.h, int(t0), t1, ptr(T, C.c_double), C.byref(p),
                                                                        rec.ctypes.data))
        return rec

    def run_disparity(self):
        """viso_batch_run_disparity: only the disparity, over the resident images (upload_images_only)."""
        self._chk("viso_batch_run_disparity", self.L.viso_batch_run_disparity(self.h))

    def disparity(self, t):
        """Frame t's int16 map [rows][cols] from the last run that computed one."""
        out = np.empty(self.image_shape(), np.int16)
        self._chk("viso_batch_get_disparity", self.L.viso_batch_get_disparity(self.h, int(t), ptr(out, C.c_int16)))
        return out

    def disparities(self):
        """Every frame's int16 map, [n_frames][rows][cols]."""
        out = np.empty((self.nf,) + tuple(self.image_shape()), np.int16)
        self._chk("viso_batch_get_disparities", self.L.viso_batch_get_disparities(self.h, ptr(out, C.c_int16)))
        return out

    def _records(self, name, dtype, t=None):
        """viso_batch_get_<name>(t): frame t's record of the last run (a 0-d array of dtype), or with t None viso_batch_get_<name>s:
        the records of all frames (structured array [n_frames], frame 0: status 0)."""
        if t is None:
            out = np.zeros(self.nf, dtype)
            self._chk(f"viso_batch_get_{name}s", getattr(self.L, f"viso_batch_get_{name}s")(self.h, out.ctypes.data))
        else:
            out = np.zeros((), dtype)
            self._chk(f"viso_batch_get_{name}", getattr(self.L, f"viso_batch_get_{name}")(self.h, int(t), out.ctypes.data))
        return out

    def set_covariance(self, mode, sigma=None):
        """viso_batch_set_covariance: 0 = off (default), 1 = per-frame motion covariance with sigma^2 estimated, 2 = with the given
        sigma (pixels), for the next runs (run, and run_images unless matcher_only)."""
        self._chk("viso_batch_set_covariance", self.L.viso_batch_set_covariance(self.h, int(mode), _sigma(sigma)))

    def covariance(self, t):
        """The motion covariance record of frame t from the last run (a 0-d MOTION_COV_DTYPE array)."""
        return self._records("covariance", MOTION_COV_DTYPE, t)

    def covariances(self):
        """The records of all frames from the last run: structured array [n_frames] of MOTION_COV_DTYPE (frame 0: status 0)."""
        return self._records("covariance", MOTION_COV_DTYPE)

    def set_refine(self, mode, sigma=None):
        """viso_batch_set_refine: 0 = off (default), 1 = two-frame bundle adjustment of every solved frame with sigma^2 estimated,
        2 = with the given sigma (pixels), for the next runs (run, and run_images unless matcher_only)."""
        self._chk("viso_batch_set_refine", self.L.viso_batch_set_refine(self.h, int(mode), _sigma(sigma)))

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
        self._chk("viso_batch_get_refined_points", self.L.viso_batch_get_refined_points(
            self.h, int(t), ptr(idx, C.c_int32), ptr(X, C.c_double), C.byref(n)))
        return idx[:n.value].copy(), X[:, :n.value].copy()

    def set_window_refine(self, K, mode=1, sigma=None):
        """viso_batch_set_window_refine: K = 0 off (default), K in 2..5 the sliding-window bundle adjustment of every solved frame
        over the window of frames t-K+1..t (mode 1: sigma^2 estimated, mode 2: the given sigma in pixels), for the next runs (run,
        and run_images unless matcher_only)."""
        self._chk("viso_batch_set_window_refine", self.L.viso_batch_set_window_refine(self.h, int(K), int(mode), _sigma(sigma)))

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
        self._chk("viso_batch_get_points",
                  self.L.viso_batch_get_points(self.h, int(t), ptr(X, C.c_double), ptr(obs, C.c_double), C.byref(m)))
        return X[:, :m.value].copy(), obs[:, :m.value].copy()

    def set_params(self, stereo, temporal, param, seed=0, first_frame=0):
        self._chk("viso_batch_set_params", self.L.viso_batch_set_params(
            self.h, C.byref(stereo), C.byref(temporal), C.byref(param), seed, first_frame))
        self.ransac_iter = int(param.ransac_iter)     # what viso_batch_get_hypotheses copies per frame

    def run_matcher(self):
        self._chk("viso_batch_run_matcher", self.L.viso_batch_run_matcher(self.h))

    def run(self):
        self._chk("viso_batch_run", self.L.viso_batch_run(self.h))

    def matches(self, which, t):
        out = np.empty((self.cap, 3), np.int32)
        n = C.c_int(0)
        self._chk("viso_batch_get_matches", self.L.viso_batch_get_matches(self.h, which, t, ptr(out, C.c_int32), C.byref(n)))
        return out[:n.value].copy()

    def circle(self, t):
        circ = np.empty((self.cap, 4), np.int32)
        pcl = np.empty((self.cap, 2), np.int32)
        n = C.c_int(0)
        self._chk("viso_batch_get_circle", self.L.viso_batch_get_circle(self.h, t, ptr(circ, C.c_int32), ptr(pcl, C.c_int32), C.byref(n)))
        return circ[:n.value].copy(), pcl[:n.value].copy()

    def pose(self, t):
        tr = np.zeros(6)
        ok, n = C.c_int(0), C.c_int(0)
        inl = np.empty(self.cap, np.int32)
        self._chk("viso_batch_get_pose", self.L.viso_batch_get_pose(self.h, t, ptr(tr, C.c_double), C.byref(ok), ptr(inl, C.c_int32), C.byref(n)))
        return ok.value, tr, inl[:n.value].copy()

    def poses(self):
        tr = np.zeros((self.nf, 6))
        ok = np.zeros(self.nf, np.int32)
        n = np.zeros(self.nf, np.int32)
        self._chk("viso_batch_get_poses", self.L.viso_batch_get_poses(self.h, ptr(tr, C.c_double), ptr(ok, C.c_int32), ptr(n, C.c_int32)))
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
        self._chk("viso_batch_get_hypotheses", self.L.viso_batch_get_hypotheses(
            self.h, ptr(tr, C.c_double), ptr(ok, C.c_int32), ptr(cnt, C.c_int32), ptr(nu, C.c_int32)))
        return tr, ok, cnt, int(nu[0])

    def counters(self):
        sc = np.zeros((3, self.nf), np.int64)
        mo = np.zeros((3, self.nf), np.int64)
        self._chk("viso_batch_get_counters", self.L.viso_batch_get_counters(self.h, ptr(sc, C.c_int64), ptr(mo, C.c_int64)))
        return sc, mo

    def general_path_flags(self):
        f = np.zeros((self.nf, 2), np.int32)
        self._chk("viso_batch_get_general_path_flags", self.L.viso_batch_get_general_path_flags(self.h, ptr(f, C.c_int32)))
        return f

    def overflow_count(self):
        n = C.c_int32(0)
        self._chk("viso_batch_get_overflow_count", self.L.viso_batch_get_overflow_count(self.h, C.byref(n)))
        return n.value

    def row8_shift(self):
        s = C.c_int(-1)
        self._chk("viso_batch_get_row8_shift", self.L.viso_batch_get_row8_shift(self.h, C.byref(s)))
        return s.value

    def kernel_timing(self, enable):
        self._chk("viso_batch_kernel_timing", self.L.viso_batch_kernel_timing(self.h, int(enable)))

    def kernel_ms(self):
        ms = C.c_double(0)
        n = C.c_int(0)
        self._chk("viso_batch_kernel_ms", self.L.viso_batch_kernel_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def device_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk("viso_batch_device_ptrs", self.L.viso_batch_device_ptrs(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def close(self):
        if self.h:
            h, self.h = self.h, None
            r = self.L.viso_batch_destroy(h)
            if r != 1:
                _err("viso_batch_destroy", r)

    def __del__(self, _finalizing=sys.is_finalizing):   # bound at definition: module globals are None late in shutdown
        if _finalizing():   # the atexit hook has closed everything that was still open
            return
        try:
            self.close()
        except Exception:
            pass
