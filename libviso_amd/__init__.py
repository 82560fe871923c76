"""libviso_amd — MI355X (gfx950) implementation of libviso's per-frame hot path.

The product is the C-ABI shared library built from libviso_amd/csrc
(libviso_hip.so, declared in include/viso_hip.h) plus the C++ host mirror of
the reference interface in libviso_amd/host.  This Python package is plumbing
for tests and bench.py: a ctypes loader and numpy-in/numpy-out wrappers with
the reference's function names.  There is NO CPU fallback: if the library is
missing, or no HIP device is present, calls raise.

This file holds the loader and what every wrapper shares; the wrappers live in sibling modules named after the csrc files
they reach (plain, dense, maps, estimators, batch, posegraph, loops) and are re-exported at the end.  The prototypes are abi.PROTOTYPES.
"""
import atexit
import ctypes as C
import os
import subprocess
import sys
import weakref

import numpy as np

from . import abi
# (the whole list is re-exported: what `from libviso_amd import ...` has always offered)
from .abi import (DESC_LEN, MAP_DEFAULTS, MAP_ENTRY_DTYPE, MOTION_COV_DTYPE, MOTION_REFINE_DTYPE, SGM_DEFAULTS, SPECKLE_DEFAULTS,  # noqa: F401
                  TSDF_ALIGN_DEFAULTS, TSDF_ALIGN_GRAY_DEFAULTS, TSDF_ALIGN_GRAY_STEP_DTYPE, TSDF_ALIGN_STEP_DTYPE, TSDF_ALIGNMENT_DTYPE,
                  TSDF_ALIGNMENT_GRAY_DTYPE, TSDF_CROSSING_DTYPE, TSDF_DEFAULTS, TSDF_ENTRY_DTYPE, TSDF_FUSE_DEFAULTS,
                  TSDF_GRAY_ENTRY_DTYPE, TSDF_MESH_VERTEX_DTYPE, TSDF_NORMAL_COUNTERS, TSDF_NORMAL_DTYPE, TSDF_NORMAL_GRAY_COUNTERS, TSDF_NORMAL_GRAY_DTYPE,
                  WINDOW_RECORD_DTYPE, DisparityParams, MapCounters, MapParams, MatchParams, Param, SgmParams, SpeckleParams,
                  TsdfAlignGrayParams, TsdfAlignParams, TsdfCounters, TsdfParams, VoxelBox, f32p, f64p, i32p, i64p, intp, ptr)

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
    abi.declare(L)
    _lib = L
    return L


def _fail(fn, code):
    raise VisoError(f"{fn.__name__} failed with {code}: {_lib.viso_last_error().decode(errors='replace')}")


def _call(fn, *args):
    """fn(*args) of the loaded library; any result but VISO_OK raises with the function's own name and viso_last_error()."""
    r = fn(*args)
    if r != 1:
        _fail(fn, r)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _sigma(sigma):
    """The sigma_px argument of the estimators: 0.0 when not given (mode 1 ignores it)."""
    return float(sigma) if sigma is not None else 0.0


def _map16(where, a):
    """A disparity map argument as a contiguous array: 2-D int16, never converted."""
    a = np.ascontiguousarray(a)
    if a.ndim != 2 or a.dtype != np.int16:
        raise ValueError(f"{where}: the map must be a 2-D int16 array")
    return a


def _image_pair(where, imgL, imgR):
    """The two images of a rectified pair as contiguous uint8 arrays."""
    imgL = np.ascontiguousarray(imgL, dtype=np.uint8)
    imgR = np.ascontiguousarray(imgR, dtype=np.uint8)
    if imgL.shape != imgR.shape or imgL.ndim != 2:
        raise ValueError(f"{where}: the two images must be 2-D and of one size")
    return imgL, imgR


def _pose_arg(where, pose, square=False):
    """A pose argument: None, or a 4 x 4 (unless square: or 3 x 4) matrix as contiguous float64 (the first three rows are read),
    and its pointer."""
    if pose is None:
        return None, None
    if square and np.shape(pose) != (4, 4):
        raise ValueError(f"{where}: the pose must be a 4 x 4 matrix")
    T = np.ascontiguousarray(pose, dtype=np.float64)
    if T.shape not in ((4, 4), (3, 4)):
        raise ValueError(f"{where}: the pose must be a 4 x 4 (or 3 x 4) matrix")
    return T, ptr(T, C.c_double)


def _params(Struct, defaults, where, fields):
    """Struct(**defaults) with `fields` replaced, each value coerced by its field's ctypes type.  Needs no library."""
    p, types = Struct(**defaults), dict(Struct._fields_)
    for k, v in fields.items():
        if k not in defaults:
            raise TypeError(f"{where}: unknown parameter {k!r}")
        setattr(p, k, float(v) if types[k] is C.c_double else int(v))
    return p


def _struct_arg(where, Struct, make, params, kw, a="a"):
    """What the calls that take parameters accept: a Struct as it is, or make(**fields) of a dict of fields and / or keyword
    fields (None and no keywords: the defaults)."""
    if isinstance(params, Struct):
        if kw:
            raise TypeError(f"{where}: keyword fields cannot be combined with {a} {Struct.__name__}")
        return params
    return make(**dict(params or {}, **kw))


# Handles that are still open when the interpreter exits are closed HERE, from an atexit hook: that runs before
# the HIP runtime's own teardown, whereas a __del__ during interpreter finalisation can run after it (calling
# hipStreamSynchronize then aborts the process from inside the runtime).  Batches and maps first, then contexts.
_live = weakref.WeakSet()


def _close_all():
    for o in sorted(_live, key=lambda o: o._close_last):
        try:
            o.close()
        except Exception:
            pass


atexit.register(_close_all)


class _Handle:
    """An object that owns one handle of the library, self.h (None once closed), freed by the C function named _destroy."""
    h, _destroy = None, None
    _close_last = False   # True: at exit, after the others (a context, whose batches and maps go first)

    def _own(self, h):
        self.h = h
        _live.add(self)

    def close(self):
        if self.h:
            h, self.h = self.h, None
            _call(getattr(self.L, self._destroy), h)

    def __del__(self, _finalizing=sys.is_finalizing):   # bound at definition: module globals are None late in shutdown
        if _finalizing():   # the atexit hook has closed everything that was still open
            return
        try:
            self.close()
        except Exception:
            pass


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


def _ctx_h(ctx):
    return ctx.h if ctx is not None else None


def set_matcher_variant(v, ctx=None):
    """Which kernel takes the temporal calls: of `ctx`, or of the plain family's default context."""
    _call(load().viso_ctx_set_matcher, _ctx_h(ctx), int(v))


def set_row8_shift(shift, ctx=None):
    """viso_ctx_set_row8_shift: the shift of match_union8_kernel's 8-bit planes, -1 = chosen from the data (default), 0..3 = fixed."""
    _call(load().viso_ctx_set_row8_shift, _ctx_h(ctx), int(shift))


def set_gn_split(split, ctx=None):
    """viso_ctx_set_gn_split: iterations of a 3-point hypothesis done by the lane-per-hypothesis kernel (0 = default)."""
    _call(load().viso_ctx_set_gn_split, _ctx_h(ctx), int(split))


def matcher_kernel_name(ctx=None):
    return load().viso_ctx_matcher_kernel_name(_ctx_h(ctx)).decode()


from .plain import (HARRIS_K, F_from_P, collect_matches, detect_harris_binned, extract_descriptors, get_inliers,  # noqa: E402,F401
                    harris_response, match_circle, match_desc, minimize_reproj, pose_update, ransac_minimize_reproj, ransac_samples,
                    refine_stereo_subpixel, support_sizes, tr2mat, triangulate_rectified)
from .dense import (DISP_INVALID, disparity_params, disparity_to_float, disparity_to_points, filter_speckles,  # noqa: E402,F401
                    rectify_images, rectify_map, sgm_frame_bytes, sgm_params, sgm_set_workspace_cap, speckle_frame_bytes, speckle_params,
                    speckle_set_workspace_cap, stereo_disparity, stereo_sgm)
from .maps import (DistanceField, TravelField, TsdfMap, TsdfNormals, VoxelMap, _box_arg, map_entry_centroids, map_params, map_ply_bytes, merge_entries,  # noqa: E402,F401
                   mesh_normals_ply_bytes, mesh_ply_bytes, shade_normals, surface_normals_ply_bytes, surface_ply_bytes,
                   write_mesh_normals_ply, write_surface_normals_ply, tsdf_align_gray_params, tsdf_align_params, tsdf_crossing_points,
                   tsdf_fuse_options, tsdf_normal_gray_matrix, tsdf_normal_matrix, tsdf_params, voxel_box, write_map_ply, write_mesh_ply,
                   write_surface_ply, travel_clearance_sq)
from .estimators import (chain_covariances, pose_covariance, pose_refine, refines_as_covariances, window_refine,  # noqa: E402,F401
                         window_refines_as_covariances)
from .batch import Batch, Context, PinnedArray  # noqa: E402,F401
from .posegraph import PoseGraph, alignment_prior, motion_edge, motion_edges, read_edges, write_edges  # noqa: E402,F401
from .loops import (batch_place_signatures, batch_wide_match, detect_loops, frame_nodes, loop_edge, loop_observations,  # noqa: E402,F401
                    place_candidates, place_scores, place_signatures, wide_match)
