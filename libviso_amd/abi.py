"""ctypes view of include/viso_hip.h: the POD structs, the records as numpy dtypes, and PROTOTYPES, the one table of every
function's restype and argtypes (declare() applies it to a loaded library; tests/test_cabi_cpu.py holds it to the header).

Test/bench plumbing only: the product is the C-ABI library itself
(libviso_amd/csrc -> libviso_hip.so) and the C++ host mirror in
libviso_amd/host.  The oracle's ctypes wrapper (oracle/pyoracle.py) reuses the
struct definitions from here; nothing here imports the oracle.
"""
import ctypes as C

import numpy as np

VISO_OK = 1
VISO_ERR_ARG = -1
VISO_ERR_HIP = -2
VISO_ERR_UNSUPPORTED = -3
VISO_ERR_NOMEM = -4
DESC_LEN = 121


class MatchParams(C.Structure):
    """struct viso_match_params <- MatchParams, reference src/viso.cpp:48-75."""
    _fields_ = [
        ("enforce_epipolar", C.c_int32),
        ("enforce_2nd_best", C.c_int32),
        ("max_neighbors", C.c_int32),
        ("_pad", C.c_int32),
        ("F", C.c_double * 9),
        ("sampson_thresh", C.c_double),
        ("ratio_2nd_best", C.c_double),
        ("radius", C.c_double),
    ]

    @classmethod
    def stereo(cls, F):
        """MatchParams(F), reference src/viso.cpp:62-71."""
        mp = cls()
        mp.enforce_epipolar = 1
        mp.sampson_thresh = 1.0
        mp.enforce_2nd_best = 0
        mp.ratio_2nd_best = 0.8
        mp.max_neighbors = 200
        mp.radius = 80.0
        Fa = np.asarray(F, dtype=np.float64).reshape(9)
        for i in range(9):
            mp.F[i] = float(Fa[i])
        return mp

    @classmethod
    def temporal(cls):
        """MatchParams(), reference src/viso.cpp:72-74."""
        mp = cls()
        mp.enforce_epipolar = 0
        mp.enforce_2nd_best = 1
        mp.ratio_2nd_best = 0.9
        mp.max_neighbors = 250
        mp.radius = 80.0
        return mp


class Param(C.Structure):
    """struct viso_param <- struct param, reference src/viso.h:58-72."""
    _fields_ = [
        ("base", C.c_double),
        ("ransac_iter", C.c_int32),
        ("save_debug", C.c_int32),
        ("inlier_threshold", C.c_double),
        ("thresh", C.c_double),
        ("f", C.c_double),
        ("cu", C.c_double),
        ("cv", C.c_double),
    ]

    @classmethod
    def default(cls, base=0.0, f=0.0, cu=0.0, cv=0.0):
        p = cls()
        p.ransac_iter = 50
        p.inlier_threshold = 2.0
        p.save_debug = 1
        p.thresh = 1e-4
        p.base, p.f, p.cu, p.cv = base, f, cu, cv
        return p

    @classmethod
    def kitti00(cls):
        """Calibration of KITTI seq 00 (values: reference test/test.cpp:11-20)."""
        return cls.default(base=386.1448 / 718.856, f=718.856, cu=607.1928, cv=185.2157)


def ptr(a, ctype):
    """Pointer to a contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return a.ctypes.data_as(C.POINTER(ctype))


f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)
i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)
u8p = C.POINTER(C.c_uint8)
intp = C.POINTER(C.c_int)


class DisparityParams(C.Structure):
    """struct viso_disparity_params (include/viso_hip.h, "dense stereo disparity")."""
    _fields_ = [(name, C.c_int32) for name in ("num_disp", "block", "prefilter_cap", "texture_threshold", "uniqueness", "lr_max_diff")]


class SgmParams(C.Structure):
    """struct viso_sgm_params (include/viso_hip.h, "semi-global matching")."""
    _fields_ = [(name, C.c_int32) for name in ("num_disp", "p1", "p2", "paths", "uniqueness", "lr_max_diff")]

    def ok(self):
        """The valid ranges of include/viso_hip.h (what the library checks before it touches a device)."""
        return (16 <= self.num_disp <= 256 and self.num_disp % 16 == 0 and 1 <= self.p1 <= self.p2 <= 192 and self.paths in (4, 8)
                and 0 <= self.uniqueness <= 100 and -1 <= self.lr_max_diff <= self.num_disp)


SGM_DEFAULTS = dict(num_disp=128, p1=10, p2=120, paths=8, uniqueness=10, lr_max_diff=1)   # viso_sgm_params_default


class SpeckleParams(C.Structure):
    """struct viso_speckle_params (include/viso_hip.h, "speckle filter and 3-D reprojection of the maps")."""
    _fields_ = [(name, C.c_int32) for name in ("max_size", "max_diff")]

    def ok(self):
        """The valid ranges of include/viso_hip.h (what the library checks before it touches a device)."""
        return self.max_size >= 0 and 0 <= self.max_diff <= 4096


SPECKLE_DEFAULTS = dict(max_size=100, max_diff=16)   # viso_speckle_params_default


class MapParams(C.Structure):
    """struct viso_map_params (include/viso_hip.h, "voxel map")."""
    _fields_ = [("voxel", C.c_double), ("min_disp16", C.c_int32), ("capacity_log2", C.c_int32)]

    def ok(self):
        """The valid ranges of include/viso_hip.h (what the library checks before it touches a device)."""
        return bool(np.isfinite(self.voxel)) and self.voxel > 0 and self.min_disp16 >= 1 and 10 <= self.capacity_log2 <= 28


MAP_DEFAULTS = dict(voxel=0.2, min_disp16=16, capacity_log2=24)   # viso_map_params_default

# struct viso_map_entry: 40 bytes
MAP_ENTRY_DTYPE = np.dtype([("k", np.int32, (3,)), ("count", np.uint32), ("sum", np.uint64, (3,))])


class MapCounters(C.Structure):
    """struct viso_map_counters (include/viso_hip.h, "voxel map")."""
    _fields_ = [(name, C.c_uint64) for name in ("n_points", "n_inserts", "n_out_of_range", "n_dropped", "n_occupied")]


class VoxelBox(C.Structure):
    """struct viso_voxel_box (include/viso_hip.h, "Map eviction")."""
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]


# include/viso_hip.h, "TSDF distance field": the flag, the state bit of a surface voxel, and sq where the box holds no site
FIELD_UNKNOWN_IS_SITE = 1
FIELD_STATE_SURFACE = 4
FIELD_NONE = 0xffffffff


class TsdfParams(C.Structure):
    """struct viso_tsdf_params (include/viso_hip.h, "TSDF map")."""
    _fields_ = [("voxel", C.c_double), ("trunc_voxels", C.c_int32), ("min_disp16", C.c_int32), ("capacity_log2", C.c_int32)]

    def ok(self):
        """The valid ranges of include/viso_hip.h (what the library checks before it touches a device)."""
        return (bool(np.isfinite(self.voxel)) and self.voxel > 0 and 1 <= self.trunc_voxels <= 8 and self.min_disp16 >= 1
                and 10 <= self.capacity_log2 <= 28)


TSDF_DEFAULTS = dict(voxel=0.2, trunc_voxels=3, min_disp16=16, capacity_log2=26)   # viso_tsdf_params_default

# struct viso_tsdf_entry (24 bytes) and struct viso_tsdf_crossing (40 bytes)
TSDF_ENTRY_DTYPE = np.dtype([("k", np.int32, (3,)), ("weight", np.uint32), ("sum", np.int64)])
TSDF_CROSSING_DTYPE = np.dtype([("k", np.int32, (3,)), ("axis", np.int32), ("wa", np.uint32), ("wb", np.uint32), ("sa", np.int64),
                                ("sb", np.int64)])
# struct viso_tsdf_mesh_vertex (32 bytes); a struct viso_tsdf_triangle is a row of a uint32 [n][3] array
TSDF_MESH_VERTEX_DTYPE = np.dtype([("k", np.int32, (3,)), ("dir", np.int32), ("p", np.float32, (3,)), ("weight", np.uint32)])
# struct viso_tsdf_gray_entry (32 bytes; include/viso_hip.h, "TSDF intensity")
TSDF_GRAY_ENTRY_DTYPE = np.dtype([("k", np.int32, (3,)), ("weight", np.uint32), ("sum", np.int64), ("gray", np.uint64)])


class TsdfCounters(C.Structure):
    """struct viso_tsdf_counters (include/viso_hip.h, "TSDF map")."""
    _fields_ = [(name, C.c_uint64) for name in ("n_points", "n_updates", "n_out_of_range", "n_dropped", "n_occupied")]


# the options of a new map, in the order of viso_tsdf_set_fuse_options' parameters (include/viso_hip.h, "TSDF fuse options")
TSDF_FUSE_DEFAULTS = dict(carve_voxels=0, weight_shift=-1, weight_max=255, carve_near=0.0)


class TsdfRetractReport(C.Structure):
    """The six uint64 a retract or a move reports, in the order of VISO_RETRACT_* (include/viso_hip.h, "TSDF retract", rule 6)."""
    _fields_ = [(name, C.c_uint64) for name in ("n_points", "n_updates", "n_missing", "n_underflow", "n_inconsistent", "n_freed")]

    def words(self):
        """The report as the calls take it: a pointer to its six words."""
        return C.cast(C.pointer(self), C.POINTER(C.c_uint64))

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class TsdfAlignParams(C.Structure):
    """struct viso_tsdf_align_params (include/viso_hip.h, "TSDF align")."""
    _fields_ = [("min_weight", C.c_uint32), ("gate_voxels", C.c_double), ("max_iters", C.c_int32), ("eps_rot", C.c_double),
                ("eps_trans", C.c_double), ("min_pixels", C.c_int32)]

    def ok(self, trunc_voxels=8):
        """The valid ranges of include/viso_hip.h for a map of trunc_voxels."""
        return (self.min_weight >= 1 and bool(np.isfinite(self.gate_voxels)) and 0 < self.gate_voxels <= trunc_voxels
                and 1 <= self.max_iters <= 50 and bool(np.isfinite(self.eps_rot)) and self.eps_rot >= 0
                and bool(np.isfinite(self.eps_trans)) and self.eps_trans >= 0 and self.min_pixels >= 6)


TSDF_ALIGN_DEFAULTS = dict(min_weight=2, gate_voxels=1.0, max_iters=10, eps_rot=1e-6, eps_trans=1e-5, min_pixels=200)   # viso_tsdf_align_params_default
TSDF_NORMAL_COUNTERS = ("n_points", "n_used", "n_missing", "n_gated", "n_clipped", "n_out_of_range")
# struct viso_tsdf_normal (272 bytes), struct viso_tsdf_alignment (440 bytes), struct viso_tsdf_align_step (400 bytes)
TSDF_NORMAL_DTYPE = np.dtype([("n", np.int64, (28,))] + [(name, np.uint64) for name in TSDF_NORMAL_COUNTERS])
TSDF_ALIGNMENT_DTYPE = np.dtype([("pose", np.float64, (4, 4)), ("cov", np.float64, (6, 6)), ("cost", np.float64), ("n_used", np.uint64),
                                 ("iters", np.int32), ("status", np.int32)])
TSDF_ALIGN_STEP_DTYPE = np.dtype([("pose", np.float64, (4, 4)), ("normal", TSDF_NORMAL_DTYPE)])


class TsdfAlignGrayParams(C.Structure):
    """struct viso_tsdf_align_gray_params (include/viso_hip.h, "TSDF photometric align")."""
    _fields_ = [("geo", TsdfAlignParams), ("photo_weight", C.c_double), ("photo_gate", C.c_double)]

    def ok(self, trunc_voxels=8):
        return (self.geo.ok(trunc_voxels) and bool(np.isfinite(self.photo_weight)) and self.photo_weight >= 0
                and bool(np.isfinite(self.photo_gate)) and self.photo_gate > 0)


TSDF_ALIGN_GRAY_DEFAULTS = dict(photo_weight=1.0 / 32.0, photo_gate=255.0)   # viso_tsdf_align_gray_params_default, beside TSDF_ALIGN_DEFAULTS
TSDF_NORMAL_GRAY_COUNTERS = ("n_photo_used", "n_photo_gated", "n_photo_clipped")
# struct viso_tsdf_normal_gray (304 bytes), struct viso_tsdf_alignment_gray (464 bytes), struct viso_tsdf_align_gray_step (432 bytes)
# (the leading struct of each is spelled out, so that a record has the plain one's fields and the new ones side by side)
TSDF_NORMAL_GRAY_DTYPE = np.dtype([("n", np.int64, (28,))] + [(name, np.uint64) for name in TSDF_NORMAL_COUNTERS] + [("p", np.int64)]
                                  + [(name, np.uint64) for name in TSDF_NORMAL_GRAY_COUNTERS])
TSDF_ALIGNMENT_GRAY_DTYPE = np.dtype([("pose", np.float64, (4, 4)), ("cov", np.float64, (6, 6)), ("cost", np.float64), ("n_used", np.uint64),
                                      ("iters", np.int32), ("status", np.int32), ("cost_geo", np.float64), ("cost_photo", np.float64),
                                      ("n_photo_used", np.uint64)])
TSDF_ALIGN_GRAY_STEP_DTYPE = np.dtype([("pose", np.float64, (4, 4)), ("normal", TSDF_NORMAL_GRAY_DTYPE)])


class MotionCov(C.Structure):
    """struct viso_motion_cov (include/viso_hip.h, "motion covariance")."""
    _fields_ = [
        ("cov", C.c_double * 36),
        ("delta", C.c_double * 6),
        ("sigma2", C.c_double),
        ("gap", C.c_double),
        ("status", C.c_int32),
        ("n", C.c_int32),
    ]


# the same layout as a numpy structured dtype (Batch.covariances, pose_covariance)
MOTION_COV_DTYPE = np.dtype([("cov", np.float64, (6, 6)), ("delta", np.float64, 6), ("sigma2", np.float64), ("gap", np.float64),
                             ("status", np.int32), ("n", np.int32)])
assert MOTION_COV_DTYPE.itemsize == C.sizeof(MotionCov) == 360


# struct viso_motion_refine (include/viso_hip.h, "motion refinement") as a numpy structured dtype (Batch.refines, pose_refine)
MOTION_REFINE_DTYPE = np.dtype([("tr", np.float64, 6), ("cov", np.float64, (6, 6)), ("sigma2", np.float64), ("cost0", np.float64),
                                ("cost", np.float64), ("gap", np.float64), ("iters", np.int32), ("status", np.int32),
                                ("n", np.int32), ("_pad", np.int32)])
assert MOTION_REFINE_DTYPE.itemsize == 384


# struct viso_window_record (include/viso_hip.h, "window refinement") as a numpy structured dtype (Batch.window_refines, window_refine)
WINDOW_RECORD_DTYPE = np.dtype([("tr", np.float64, 6), ("cov", np.float64, (6, 6)), ("tr_win", np.float64, (4, 6)),
                                ("sigma2", np.float64), ("cost0", np.float64), ("cost", np.float64), ("gap", np.float64),
                                ("iters", np.int32), ("status", np.int32), ("len", np.int32), ("n_points", np.int32),
                                ("n_rows", np.int32), ("_pad", np.int32)])
assert WINDOW_RECORD_DTYPE.itemsize == 584


class PlainTimes(C.Structure):
    """struct viso_plain_times (include/viso_hip.h, "plain (host) family"): viso_plain_profile_get."""
    _fields_ = [("calls", C.c_int64), ("host_us", C.c_double), ("h2d_us", C.c_double), ("kernel_us", C.c_double),
                ("d2h_us", C.c_double), ("wait_us", C.c_double)]


# ------------------------------------------------------------ prototypes
# Every function include/viso_hip.h declares, name without the viso_ prefix -> (restype, [argtypes]), in the header's order and
# under its section names.  Handles (viso_ctx*, viso_batch*, viso_map*, viso_tsdf*) and pointers to the records that are numpy
# dtypes here are vp; a pointer to a struct with a ctypes class is P(that class).  tests/test_cabi_cpu.py parses the header
# and holds every entry to it.
P = C.POINTER
i, i64, u32, u64, sz, dbl, vp = C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_size_t, C.c_double, C.c_void_p
i16p, u32p, u64p, szp, vpp = P(C.c_int16), P(C.c_uint32), P(C.c_uint64), P(C.c_size_t), P(C.c_void_p)
MP, PP = P(MatchParams), P(Param)

PROTOTYPES = {
    # parameter constructors (ahead of the first section)
    "match_params_stereo": (None, [MP, f64p]),
    "match_params_temporal": (None, [MP]),
    "param_default": (None, [PP]),
    # context
    "ctx_create": (vp, [i, vp]),
    "ctx_destroy": (i, [vp]),
    "ctx_stream": (vp, [vp]),
    "ctx_synchronize": (i, [vp]),
    "ctx_set_matcher": (i, [vp, i]),
    "matcher_variants": (i, [intp, i]),
    "matcher_default": (i, []),
    "ctx_set_gn_split": (i, [vp, i]),
    "ctx_set_row8_shift": (i, [vp, i]),
    "ctx_matcher_kernel_name": (C.c_char_p, [vp]),
    "last_error": (C.c_char_p, []),
    "version": (C.c_char_p, []),
    # plain (host) family
    "match_desc": (i, [f32p, i, f32p, i, f32p, f32p, i, MP, i32p, intp]),
    "match_circle": (i, [i32p, i, i32p, i, i32p, i, i32p, i, i32p, i32p, i, intp]),
    "collect_matches": (i, [f32p, i, f32p, i, i32p, i, f64p]),
    "triangulate_rectified": (i, [f64p, i, PP, f64p]),
    "minimize_reproj": (i, [f64p, f64p, i, f64p, PP, i32p, i]),
    "get_inliers": (i, [f64p, f64p, i, f64p, PP, i32p, intp, f64p]),
    "ransac_minimize_reproj": (i, [f64p, f64p, i, f64p, i32p, intp, PP, i32p, u64, u64]),
    "support_sizes": (i, [f64p, f64p, i, f64p, i, PP, i32p]),
    "ransac_samples": (None, [u64, u64, i, i, i32p]),
    "tr2mat": (None, [f64p, f64p]),
    "pose_update": (None, [f64p, f64p, f64p]),
    "F_from_P": (None, [f64p, f64p, f64p]),
    "extract_descriptors": (i, [u8p, i, i, f32p, i, i, f32p]),
    "harris_response": (i, [u8p, i, i, dbl, f32p]),
    "detect_harris_binned": (i, [u8p, i, i, i, i, i, dbl, f32p, f32p, intp]),
    "plain_cache": (i, [i]),
    "plain_cache_stats": (i, [i64p, i64p]),
    "plain_general_reruns": (i64, []),
    "plain_speculate": (i, [i]),
    "plain_speculate_stats": (i, [i64p]),
    "plain_trace_dump": (None, []),
    "plain_profile": (i, [i]),
    "plain_profile_get": (i, [i, P(PlainTimes)]),
    "plain_profile_name": (C.c_char_p, [i]),
    # batched, device-resident family
    "batch_create": (vp, [vp, i, i, i]),
    "batch_destroy": (i, [vp]),
    "batch_upload": (i, [vp, i, i, f32p, f32p, i32p]),
    "batch_upload_async": (i, [vp, i, i, f32p, f32p, i32p]),
    "batch_upload_i16": (i, [vp, i, i, f32p, i16p, i32p]),
    "batch_upload_i16_async": (i, [vp, i, i, f32p, i16p, i32p]),
    "host_alloc": (vp, [sz]),
    "host_free": (i, [vp]),
    "batch_device_ptrs": (i, [vp, vpp, vpp, vpp]),
    "batch_set_params": (i, [vp, MP, MP, PP, u64, u64]),
    "batch_run_matcher": (i, [vp]),
    "batch_run": (i, [vp]),
    "batch_upload_images": (i, [vp, i, i, u8p, i, i, f32p, i32p]),
    "batch_run_images": (i, [vp, i]),
    "batch_upload_images_async": (i, [vp, i, i, u8p, i, i, f32p, i32p]),
    "batch_detect": (i, [vp, i, i, i, dbl]),
    "batch_get_keypoints": (i, [vp, i, i, f32p, intp]),
    "batch_get_matches": (i, [vp, i, i, i32p, intp]),
    "batch_get_circle": (i, [vp, i, i32p, i32p, intp]),
    "batch_get_pose": (i, [vp, i, f64p, intp, i32p, intp]),
    "batch_get_poses": (i, [vp, f64p, i32p, i32p]),
    "batch_get_hypotheses": (i, [vp, f64p, i32p, i32p, i32p]),
    "batch_get_hypotheses2": (i, [vp, i, f64p, i32p, i32p, i32p]),
    "batch_get_counters": (i, [vp, i64p, i64p]),
    "batch_get_general_path_flags": (i, [vp, i32p]),
    "batch_get_overflow_count": (i, [vp, i32p]),
    "batch_get_row8_shift": (i, [vp, intp]),
    "batch_kernel_timing": (i, [vp, i]),
    "batch_kernel_ms": (i, [vp, f64p, intp]),
    "batch_stamp": (i, [vp, i]),
    "batch_stamp_ms": (i, [vp, f64p]),
    # sub-pixel stereo refinement
    "batch_set_subpixel": (i, [vp, i]),
    "batch_get_subpixel": (i, [vp, i, f32p, intp]),
    "refine_stereo_subpixel": (i, [u8p, u8p, i, i, f32p, i, f32p, i, i32p, i, i, f32p]),
    # rectification of raw camera images
    "rectify_map": (i, [f64p, f64p, f64p, f64p, i, i, f32p, f32p]),
    "batch_set_rectify": (i, [vp, i, i, i, i, f32p, f32p, f32p, f32p, i]),
    "batch_get_image": (i, [vp, i, i, u8p]),
    "batch_get_image_geometry": (i, [vp, intp, intp]),
    "rectify_images": (i, [u8p, i, i, i, f32p, f32p, i, i, i, u8p]),
    # motion covariance
    "batch_set_covariance": (i, [vp, i, dbl]),
    "batch_get_covariance": (i, [vp, i, vp]),
    "batch_get_covariances": (i, [vp, vp]),
    "batch_get_points": (i, [vp, i, f64p, f64p, intp]),
    "pose_covariance": (i, [f64p, f64p, i, f64p, i32p, i, PP, i, dbl, vp]),
    "chain_covariances": (i, [f64p, i32p, vp, i, f64p, i32p, intp]),
    # motion refinement
    "batch_set_refine": (i, [vp, i, dbl]),
    "batch_get_refine": (i, [vp, i, vp]),
    "batch_get_refines": (i, [vp, vp]),
    "batch_get_refined_points": (i, [vp, i, i32p, f64p, intp]),
    "pose_refine": (i, [f64p, f64p, i, f64p, i32p, i, PP, i, dbl, vp, f64p]),
    # window refinement
    "batch_set_window_refine": (i, [vp, i, i, dbl]),
    "batch_get_window_refine": (i, [vp, i, vp]),
    "batch_get_window_refines": (i, [vp, vp]),
    "window_refine": (i, [i, intp, f64p, f64p, i32p, f64p, i32p, intp, PP, i, dbl, vp]),
    # dense stereo disparity
    "disparity_params_default": (None, [P(DisparityParams)]),
    "stereo_disparity": (i, [u8p, u8p, i, i, P(DisparityParams), i16p]),
    "batch_set_disparity": (i, [vp, P(DisparityParams)]),
    "batch_run_disparity": (i, [vp]),
    "batch_get_disparity": (i, [vp, i, i16p]),
    "batch_get_disparities": (i, [vp, i16p]),
    # semi-global matching
    "sgm_params_default": (None, [P(SgmParams)]),
    "stereo_sgm": (i, [u8p, u8p, i, i, P(SgmParams), i16p]),
    "batch_set_sgm": (i, [vp, P(SgmParams)]),
    "sgm_set_workspace_cap": (None, [sz]),
    # speckle filter and 3-D reprojection of the maps
    "speckle_params_default": (None, [P(SpeckleParams)]),
    "filter_speckles": (i, [i16p, i, i, P(SpeckleParams)]),
    "batch_set_speckle": (i, [vp, P(SpeckleParams)]),
    "speckle_set_workspace_cap": (None, [sz]),
    "disparity_to_points": (i, [i16p, i, i, PP, f64p, i, f32p]),
    "batch_get_disparity_points": (i, [vp, i, f64p, i, f32p]),
    # voxel map
    "map_params_default": (None, [P(MapParams)]),
    "map_create": (i, [vp, P(MapParams), vpp]),
    "map_destroy": (i, [vp]),
    "map_clear": (i, [vp]),
    "map_fuse": (i, [vp, i16p, i, i, PP, f64p]),
    "batch_fuse_disparities": (i, [vp, vp, i, i, f64p]),
    "map_add_entries": (i, [vp, vp, sz]),
    "map_count": (i, [vp, u32, szp]),
    "map_get": (i, [vp, u32, vp, sz, szp]),
    "map_stats": (i, [vp, P(MapCounters)]),
    "map_entry_centroid": (i, [vp, dbl, f32p]),
    # TSDF map
    "tsdf_params_default": (None, [P(TsdfParams)]),
    "tsdf_create": (i, [vp, P(TsdfParams), vpp]),
    "tsdf_destroy": (i, [vp]),
    "tsdf_clear": (i, [vp]),
    "tsdf_fuse": (i, [vp, i16p, i, i, PP, f64p]),
    "batch_fuse_tsdf": (i, [vp, vp, i, i, f64p]),
    "tsdf_add_entries": (i, [vp, vp, sz]),
    "tsdf_count": (i, [vp, u32, szp]),
    "tsdf_get": (i, [vp, u32, vp, sz, szp]),
    "tsdf_surface_count": (i, [vp, u32, szp]),
    "tsdf_surface": (i, [vp, u32, vp, sz, szp]),
    "tsdf_stats": (i, [vp, P(TsdfCounters)]),
    "tsdf_crossing_point": (i, [vp, dbl, f32p]),
    # TSDF fuse options
    "tsdf_set_fuse_options": (i, [vp, C.c_int32, C.c_int32, u32, dbl]),
    "tsdf_get_fuse_options": (i, [vp, i32p, i32p, u32p, f64p]),
    # TSDF mesh
    "tsdf_mesh_count": (i, [vp, u32, szp, szp]),
    "tsdf_mesh": (i, [vp, u32, vp, sz, vp, sz, szp, szp]),
    # TSDF render
    "tsdf_render": (i, [vp, u32, PP, i, i, dbl, f64p, i, i16p, u32p]),
    # TSDF intensity
    "tsdf_create_gray": (i, [vp, P(TsdfParams), vpp]),
    "tsdf_is_gray": (i, [vp, intp]),
    "tsdf_fuse_gray": (i, [vp, i16p, u8p, i, i, PP, f64p]),
    "tsdf_get_gray": (i, [vp, u32, vp, sz, szp]),
    "tsdf_add_gray_entries": (i, [vp, vp, sz]),
    "tsdf_vertex_gray": (i, [vp, vp, sz, u8p, szp]),
    "tsdf_render_gray": (i, [vp, u32, PP, i, i, dbl, f64p, i, i16p, u32p, u8p]),
    # TSDF normals
    "tsdf_vertex_normals": (i, [vp, u32, vp, sz, f32p, szp]),
    "tsdf_render_normals": (i, [vp, u32, PP, i, i, dbl, f64p, i, i16p, u32p, f32p]),
    # TSDF align
    "tsdf_align_params_default": (None, [P(TsdfAlignParams)]),
    "tsdf_linearize": (i, [vp, P(TsdfAlignParams), i16p, i, i, PP, f64p, vp]),
    "tsdf_align": (i, [vp, P(TsdfAlignParams), i16p, i, i, PP, f64p, vp, vp, i]),
    "batch_align_tsdf": (i, [vp, vp, i, i, f64p, P(TsdfAlignParams), vp]),
    # TSDF photometric align
    "tsdf_align_gray_params_default": (None, [P(TsdfAlignGrayParams)]),
    "tsdf_linearize_gray": (i, [vp, P(TsdfAlignGrayParams), i16p, u8p, i, i, PP, f64p, vp]),
    "tsdf_align_gray": (i, [vp, P(TsdfAlignGrayParams), i16p, u8p, i, i, PP, f64p, vp, vp, i]),
    "batch_align_tsdf_gray": (i, [vp, vp, i, i, f64p, P(TsdfAlignGrayParams), vp]),
    # Map eviction
    "voxel_box_around": (i, [f64p, dbl, dbl, P(VoxelBox)]),
    "map_evict_count": (i, [vp, P(VoxelBox), szp]),
    "map_evict": (i, [vp, P(VoxelBox), vp, sz, szp]),
    "tsdf_evict_count": (i, [vp, P(VoxelBox), szp]),
    "tsdf_evict": (i, [vp, P(VoxelBox), vp, sz, szp]),
    "tsdf_evict_gray": (i, [vp, P(VoxelBox), vp, sz, szp]),
    # TSDF distance field
    "tsdf_distance_field": (i, [vp, u32, P(VoxelBox), u32, u32p, u8p, sz, szp]),
    # TSDF travel field
    "tsdf_travel_field": (i, [vp, u32, P(VoxelBox), u32, u32, i32p, sz, u32p, u32p, u8p, sz, szp, szp, szp]),
    # TSDF retract
    "tsdf_retract": (i, [vp, i16p, i, i, PP, f64p, u64p]),
    "tsdf_retract_gray": (i, [vp, i16p, u8p, i, i, PP, f64p, u64p]),
    "batch_retract_tsdf": (i, [vp, vp, i, i, f64p, u64p]),
    "tsdf_move": (i, [vp, i16p, i, i, PP, f64p, f64p, u64p]),
    "tsdf_move_gray": (i, [vp, i16p, u8p, i, i, PP, f64p, f64p, u64p]),
    "batch_move_tsdf": (i, [vp, vp, i, i, f64p, f64p, u64p]),
    # pose graph
    "pose_graph_linearize": (i, [vp, i, f64p, i32p, i, i32p, f64p, f64p, dbl, f64p, f64p, f64p]),
    "pose_graph_optimize": (i, [vp, i, f64p, i32p, i, i32p, f64p, f64p, i, dbl, f64p, f64p, f64p, i]),
    "motion_edge": (i, [f64p, f64p, f64p, f64p]),
    # loop closure
    "place_signatures": (i, [vp, i16p, i32p, i, i, u64, i, u8p]),
    "batch_place_signatures": (i, [vp, i, i, u64, i, u8p]),
    "place_scores": (i, [vp, u8p, i, i, i, u32p]),
    "place_candidates": (i, [vp, u8p, i, i, i, i, i, i, u32, i, i32p, u32p]),
    "wide_match": (i, [vp, i16p, i32p, i, i, i32p, i, dbl, i32p, i32p]),
    "batch_wide_match": (i, [vp, i32p, i, dbl, i32p, i32p]),
}

# the words of viso_pose_graph_optimize's report, in the order of VISO_PG_* (include/viso_hip.h, "pose graph")
POSE_GRAPH_REPORT = ("status", "iters", "cost_initial", "cost_final", "lambda", "last_step", "n_long", "n_rejected")

# what the oracle library exports under its own prefix with the same signatures (declare_common, oracle/pyoracle.py)
COMMON = ("match_circle", "collect_matches", "triangulate_rectified", "get_inliers", "ransac_minimize_reproj", "ransac_samples",
          "tr2mat", "pose_update", "F_from_P", "extract_descriptors")


def declare(lib, prefix="viso_", names=None):
    """Give the functions of PROTOTYPES (all, or `names`) their restype and argtypes on `lib`.  A function the library lacks is
    skipped: an older build of it (VISO_HIP_SO, A/B runs) has fewer, and tests/test_cabi_cpu.py holds the current build to the
    header's list."""
    for name in PROTOTYPES if names is None else names:
        fn = getattr(lib, prefix + name, None)
        if fn is not None:
            fn.restype, fn.argtypes = PROTOTYPES[name]


def declare_common(lib, prefix):
    """The COMMON subset of the table under `prefix`, and the two struct pointer types its callers declare their own
    functions with: what oracle/pyoracle.py asks for its library (prefix 'oracle_')."""
    declare(lib, prefix, COMMON)
    return MP, PP
