"""ctypes view of include/viso_hip.h (POD structs + prototypes).

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


def declare_common(lib, prefix):
    """Prototypes shared by libviso_hip.so (prefix 'viso_') and the oracle
    (prefix 'oracle_'): same POD signatures, include/viso_hip.h."""
    def fn(name, restype, argtypes):
        f = getattr(lib, prefix + name)
        f.restype = restype
        f.argtypes = argtypes
        return f

    MP = C.POINTER(MatchParams)
    PP = C.POINTER(Param)
    fn("match_circle", C.c_int, [i32p, C.c_int, i32p, C.c_int, i32p, C.c_int, i32p, C.c_int,
                                  i32p, i32p, C.c_int, intp])
    fn("collect_matches", C.c_int, [f32p, C.c_int, f32p, C.c_int, i32p, C.c_int, f64p])
    fn("triangulate_rectified", C.c_int, [f64p, C.c_int, PP, f64p])
    fn("get_inliers", C.c_int, [f64p, f64p, C.c_int, f64p, PP, i32p, intp, f64p])
    fn("ransac_minimize_reproj", C.c_int, [f64p, f64p, C.c_int, f64p, i32p, intp, PP, i32p,
                                           C.c_uint64, C.c_uint64])
    fn("ransac_samples", None, [C.c_uint64, C.c_uint64, C.c_int, C.c_int, i32p])
    fn("tr2mat", None, [f64p, f64p])
    fn("pose_update", None, [f64p, f64p, f64p])
    fn("F_from_P", None, [f64p, f64p, f64p])
    fn("extract_descriptors", C.c_int, [u8p, C.c_int, C.c_int, f32p, C.c_int, C.c_int, f32p])
    return MP, PP


def declare_subpixel(lib):
    """Prototypes of the opt-in sub-pixel stereo refinement (include/viso_hip.h; libviso_hip.so only)."""
    u8p = C.POINTER(C.c_uint8)
    lib.viso_batch_set_subpixel.argtypes = [C.c_void_p, C.c_int]
    lib.viso_batch_get_subpixel.argtypes = [C.c_void_p, C.c_int, f32p, intp]
    lib.viso_refine_stereo_subpixel.argtypes = [u8p, u8p, C.c_int, C.c_int, f32p, C.c_int, f32p, C.c_int, i32p, C.c_int,
                                                C.c_int, f32p]


def declare_rectify(lib):
    """Prototypes of the opt-in rectification of raw images (include/viso_hip.h; libviso_hip.so only)."""
    u8p = C.POINTER(C.c_uint8)
    lib.viso_rectify_map.argtypes = [f64p, f64p, f64p, f64p, C.c_int, C.c_int, f32p, f32p]
    lib.viso_batch_set_rectify.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, f32p, f32p, f32p, f32p, C.c_int]
    lib.viso_batch_get_image.argtypes = [C.c_void_p, C.c_int, C.c_int, u8p]
    lib.viso_batch_get_image_geometry.argtypes = [C.c_void_p, intp, intp]
    lib.viso_rectify_images.argtypes = [u8p, C.c_int, C.c_int, C.c_int, f32p, f32p, C.c_int, C.c_int, C.c_int, u8p]


class DisparityParams(C.Structure):
    """struct viso_disparity_params (include/viso_hip.h, "dense stereo disparity")."""
    _fields_ = [(name, C.c_int32) for name in ("num_disp", "block", "prefilter_cap", "texture_threshold", "uniqueness", "lr_max_diff")]


def declare_disparity(lib):
    """Prototypes of the opt-in dense disparity (include/viso_hip.h; libviso_hip.so only)."""
    u8p, i16p, DP = C.POINTER(C.c_uint8), C.POINTER(C.c_int16), C.POINTER(DisparityParams)
    lib.viso_disparity_params_default.restype = None
    lib.viso_disparity_params_default.argtypes = [DP]
    lib.viso_stereo_disparity.argtypes = [u8p, u8p, C.c_int, C.c_int, DP, i16p]
    lib.viso_batch_set_disparity.argtypes = [C.c_void_p, DP]
    lib.viso_batch_run_disparity.argtypes = [C.c_void_p]
    lib.viso_batch_get_disparity.argtypes = [C.c_void_p, C.c_int, i16p]
    lib.viso_batch_get_disparities.argtypes = [C.c_void_p, i16p]


class SgmParams(C.Structure):
    """struct viso_sgm_params (include/viso_hip.h, "semi-global matching")."""
    _fields_ = [(name, C.c_int32) for name in ("num_disp", "p1", "p2", "paths", "uniqueness", "lr_max_diff")]

    def ok(self):
        """The valid ranges of include/viso_hip.h (what the library checks before it touches a device)."""
        return (16 <= self.num_disp <= 256 and self.num_disp % 16 == 0 and 1 <= self.p1 <= self.p2 <= 192 and self.paths in (4, 8)
                and 0 <= self.uniqueness <= 100 and -1 <= self.lr_max_diff <= self.num_disp)


SGM_DEFAULTS = dict(num_disp=128, p1=10, p2=120, paths=8, uniqueness=10, lr_max_diff=1)   # viso_sgm_params_default


def declare_sgm(lib):
    """Prototypes of the opt-in semi-global matching (include/viso_hip.h; libviso_hip.so only)."""
    u8p, i16p, SP = C.POINTER(C.c_uint8), C.POINTER(C.c_int16), C.POINTER(SgmParams)
    lib.viso_sgm_params_default.restype = None
    lib.viso_sgm_params_default.argtypes = [SP]
    lib.viso_stereo_sgm.argtypes = [u8p, u8p, C.c_int, C.c_int, SP, i16p]
    lib.viso_batch_set_sgm.argtypes = [C.c_void_p, SP]
    lib.viso_sgm_set_workspace_cap.restype = None
    lib.viso_sgm_set_workspace_cap.argtypes = [C.c_size_t]


class SpeckleParams(C.Structure):
    """struct viso_speckle_params (include/viso_hip.h, "speckle filter and 3-D reprojection of the maps")."""
    _fields_ = [(name, C.c_int32) for name in ("max_size", "max_diff")]

    def ok(self):
        """The valid ranges of include/viso_hip.h (what the library checks before it touches a device)."""
        return self.max_size >= 0 and 0 <= self.max_diff <= 4096


SPECKLE_DEFAULTS = dict(max_size=100, max_diff=16)   # viso_speckle_params_default


def declare_speckle(lib):
    """Prototypes of the opt-in speckle filter and reprojection (include/viso_hip.h; libviso_hip.so only)."""
    i16p, KP = C.POINTER(C.c_int16), C.POINTER(SpeckleParams)
    lib.viso_speckle_params_default.restype = None
    lib.viso_speckle_params_default.argtypes = [KP]
    lib.viso_filter_speckles.argtypes = [i16p, C.c_int, C.c_int, KP]
    lib.viso_batch_set_speckle.argtypes = [C.c_void_p, KP]
    lib.viso_speckle_set_workspace_cap.restype = None
    lib.viso_speckle_set_workspace_cap.argtypes = [C.c_size_t]
    lib.viso_disparity_to_points.argtypes = [i16p, C.c_int, C.c_int, C.POINTER(Param), f64p, C.c_int, f32p]
    lib.viso_batch_get_disparity_points.argtypes = [C.c_void_p, C.c_int, f64p, C.c_int, f32p]


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


def declare_map(lib):
    """Prototypes of the opt-in voxel map (include/viso_hip.h; libviso_hip.so only)."""
    i16p, MPP, vp = C.POINTER(C.c_int16), C.POINTER(MapParams), C.c_void_p
    lib.viso_map_params_default.restype = None
    lib.viso_map_params_default.argtypes = [MPP]
    lib.viso_map_create.argtypes = [vp, MPP, C.POINTER(vp)]
    lib.viso_map_destroy.argtypes = [vp]
    lib.viso_map_clear.argtypes = [vp]
    lib.viso_map_fuse.argtypes = [vp, i16p, C.c_int, C.c_int, C.POINTER(Param), f64p]
    lib.viso_batch_fuse_disparities.argtypes = [vp, vp, C.c_int, C.c_int, f64p]
    lib.viso_map_add_entries.argtypes = [vp, vp, C.c_size_t]
    lib.viso_map_count.argtypes = [vp, C.c_uint32, C.POINTER(C.c_size_t)]
    lib.viso_map_get.argtypes = [vp, C.c_uint32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.viso_map_stats.argtypes = [vp, C.POINTER(MapCounters)]
    lib.viso_map_entry_centroid.argtypes = [vp, C.c_double, f32p]


class VoxelBox(C.Structure):
    """struct viso_voxel_box (include/viso_hip.h, "Map eviction")."""
    _fields_ = [("lo", C.c_int32 * 3), ("hi", C.c_int32 * 3)]


def declare_evict(lib):
    """Prototypes of the maps' eviction (include/viso_hip.h, "Map eviction")."""
    vp, szp, BP = C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(VoxelBox)
    lib.viso_voxel_box_around.argtypes = [f64p, C.c_double, C.c_double, BP]
    for kind in ("map", "tsdf"):
        getattr(lib, f"viso_{kind}_evict_count").argtypes = [vp, BP, szp]
        getattr(lib, f"viso_{kind}_evict").argtypes = [vp, BP, vp, C.c_size_t, szp]
    lib.viso_tsdf_evict_gray.argtypes = [vp, BP, vp, C.c_size_t, szp]


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


def declare_tsdf(lib):
    """Prototypes of the opt-in TSDF map (include/viso_hip.h; libviso_hip.so only)."""
    i16p, TPP, vp, szp = C.POINTER(C.c_int16), C.POINTER(TsdfParams), C.c_void_p, C.POINTER(C.c_size_t)
    lib.viso_tsdf_params_default.restype = None
    lib.viso_tsdf_params_default.argtypes = [TPP]
    lib.viso_tsdf_create.argtypes = [vp, TPP, C.POINTER(vp)]
    lib.viso_tsdf_destroy.argtypes = [vp]
    lib.viso_tsdf_clear.argtypes = [vp]
    lib.viso_tsdf_fuse.argtypes = [vp, i16p, C.c_int, C.c_int, C.POINTER(Param), f64p]
    lib.viso_batch_fuse_tsdf.argtypes = [vp, vp, C.c_int, C.c_int, f64p]
    lib.viso_tsdf_add_entries.argtypes = [vp, vp, C.c_size_t]
    lib.viso_tsdf_count.argtypes = [vp, C.c_uint32, szp]
    lib.viso_tsdf_get.argtypes = [vp, C.c_uint32, vp, C.c_size_t, szp]
    lib.viso_tsdf_surface_count.argtypes = [vp, C.c_uint32, szp]
    lib.viso_tsdf_surface.argtypes = [vp, C.c_uint32, vp, C.c_size_t, szp]
    lib.viso_tsdf_stats.argtypes = [vp, C.POINTER(TsdfCounters)]
    lib.viso_tsdf_crossing_point.argtypes = [vp, C.c_double, f32p]
    lib.viso_tsdf_mesh_count.argtypes = [vp, C.c_uint32, szp, szp]
    lib.viso_tsdf_mesh.argtypes = [vp, C.c_uint32, vp, C.c_size_t, vp, C.c_size_t, szp, szp]
    lib.viso_tsdf_render.argtypes = [vp, C.c_uint32, C.POINTER(Param), C.c_int, C.c_int, C.c_double, f64p, C.c_int, i16p,
                                     C.POINTER(C.c_uint32)]
    if hasattr(lib, "viso_tsdf_create_gray"):   # (absent from older builds of the library: VISO_HIP_SO A/B runs)
        declare_tsdf_gray(lib)
    if hasattr(lib, "viso_tsdf_linearize"):
        declare_tsdf_align(lib)
    if hasattr(lib, "viso_tsdf_linearize_gray"):
        declare_tsdf_align_gray(lib)


def declare_tsdf_gray(lib):
    """Prototypes of the gray TSDF map (include/viso_hip.h, "TSDF intensity")."""
    i16p, u8p, vp, szp = C.POINTER(C.c_int16), C.POINTER(C.c_uint8), C.c_void_p, C.POINTER(C.c_size_t)
    lib.viso_tsdf_create_gray.argtypes = [vp, C.POINTER(TsdfParams), C.POINTER(vp)]
    lib.viso_tsdf_is_gray.argtypes = [vp, C.POINTER(C.c_int)]
    lib.viso_tsdf_fuse_gray.argtypes = [vp, i16p, u8p, C.c_int, C.c_int, C.POINTER(Param), f64p]
    lib.viso_tsdf_get_gray.argtypes = [vp, C.c_uint32, vp, C.c_size_t, szp]
    lib.viso_tsdf_add_gray_entries.argtypes = [vp, vp, C.c_size_t]
    lib.viso_tsdf_vertex_gray.argtypes = [vp, vp, C.c_size_t, u8p, szp]
    lib.viso_tsdf_render_gray.argtypes = [vp, C.c_uint32, C.POINTER(Param), C.c_int, C.c_int, C.c_double, f64p, C.c_int, i16p,
                                          C.POINTER(C.c_uint32), u8p]


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


def declare_tsdf_align(lib):
    """Prototypes of the frame-to-model alignment (include/viso_hip.h, "TSDF align")."""
    i16p, vp, APP = C.POINTER(C.c_int16), C.c_void_p, C.POINTER(TsdfAlignParams)
    lib.viso_tsdf_align_params_default.restype = None
    lib.viso_tsdf_align_params_default.argtypes = [APP]
    lib.viso_tsdf_linearize.argtypes = [vp, APP, i16p, C.c_int, C.c_int, C.POINTER(Param), f64p, vp]
    lib.viso_tsdf_align.argtypes = [vp, APP, i16p, C.c_int, C.c_int, C.POINTER(Param), f64p, vp, vp, C.c_int]
    lib.viso_batch_align_tsdf.argtypes = [vp, vp, C.c_int, C.c_int, f64p, APP, vp]


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


def declare_tsdf_align_gray(lib):
    """Prototypes of the photometric frame-to-model alignment (include/viso_hip.h, "TSDF photometric align")."""
    i16p, u8p, vp, GPP = C.POINTER(C.c_int16), C.POINTER(C.c_uint8), C.c_void_p, C.POINTER(TsdfAlignGrayParams)
    lib.viso_tsdf_align_gray_params_default.restype = None
    lib.viso_tsdf_align_gray_params_default.argtypes = [GPP]
    lib.viso_tsdf_linearize_gray.argtypes = [vp, GPP, i16p, u8p, C.c_int, C.c_int, C.POINTER(Param), f64p, vp]
    lib.viso_tsdf_align_gray.argtypes = [vp, GPP, i16p, u8p, C.c_int, C.c_int, C.POINTER(Param), f64p, vp, vp, C.c_int]
    lib.viso_batch_align_tsdf_gray.argtypes = [vp, vp, C.c_int, C.c_int, f64p, GPP, vp]


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


def declare_covariance(lib):
    """Prototypes of the opt-in motion covariance (include/viso_hip.h; libviso_hip.so only)."""
    vp = C.c_void_p
    lib.viso_batch_set_covariance.argtypes = [vp, C.c_int, C.c_double]
    lib.viso_batch_get_covariance.argtypes = [vp, C.c_int, vp]
    lib.viso_batch_get_covariances.argtypes = [vp, vp]
    lib.viso_batch_get_points.argtypes = [vp, C.c_int, f64p, f64p, intp]
    lib.viso_pose_covariance.argtypes = [f64p, f64p, C.c_int, f64p, i32p, C.c_int, C.POINTER(Param), C.c_int, C.c_double, vp]
    lib.viso_chain_covariances.argtypes = [f64p, i32p, vp, C.c_int, f64p, i32p, intp]


# struct viso_motion_refine (include/viso_hip.h, "motion refinement") as a numpy structured dtype (Batch.refines, pose_refine)
MOTION_REFINE_DTYPE = np.dtype([("tr", np.float64, 6), ("cov", np.float64, (6, 6)), ("sigma2", np.float64), ("cost0", np.float64),
                                ("cost", np.float64), ("gap", np.float64), ("iters", np.int32), ("status", np.int32),
                                ("n", np.int32), ("_pad", np.int32)])
assert MOTION_REFINE_DTYPE.itemsize == 384


def declare_refine(lib):
    """Prototypes of the opt-in motion refinement (include/viso_hip.h; libviso_hip.so only)."""
    vp = C.c_void_p
    lib.viso_batch_set_refine.argtypes = [vp, C.c_int, C.c_double]
    lib.viso_batch_get_refine.argtypes = [vp, C.c_int, vp]
    lib.viso_batch_get_refines.argtypes = [vp, vp]
    lib.viso_batch_get_refined_points.argtypes = [vp, C.c_int, i32p, f64p, intp]
    lib.viso_pose_refine.argtypes = [f64p, f64p, C.c_int, f64p, i32p, C.c_int, C.POINTER(Param), C.c_int, C.c_double, vp, f64p]


# struct viso_window_record (include/viso_hip.h, "window refinement") as a numpy structured dtype (Batch.window_refines, window_refine)
WINDOW_RECORD_DTYPE = np.dtype([("tr", np.float64, 6), ("cov", np.float64, (6, 6)), ("tr_win", np.float64, (4, 6)),
                                ("sigma2", np.float64), ("cost0", np.float64), ("cost", np.float64), ("gap", np.float64),
                                ("iters", np.int32), ("status", np.int32), ("len", np.int32), ("n_points", np.int32),
                                ("n_rows", np.int32), ("_pad", np.int32)])
assert WINDOW_RECORD_DTYPE.itemsize == 584


def declare_window(lib):
    """Prototypes of the opt-in window refinement (include/viso_hip.h; libviso_hip.so only)."""
    vp = C.c_void_p
    lib.viso_batch_set_window_refine.argtypes = [vp, C.c_int, C.c_int, C.c_double]
    lib.viso_batch_get_window_refine.argtypes = [vp, C.c_int, vp]
    lib.viso_batch_get_window_refines.argtypes = [vp, vp]
    lib.viso_window_refine.argtypes = [C.c_int, intp, f64p, f64p, i32p, f64p, i32p, intp, C.POINTER(Param), C.c_int, C.c_double, vp]
