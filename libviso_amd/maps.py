"""The two maps of include/viso_hip.h, VoxelMap and TsdfMap (csrc/voxelmap.hip, tsdf.hip, tsdf_align.hip over the table layer of
csrc/voxel_host.hip): their parameters, eviction boxes, entry arithmetic on the host, and the PLY writers."""
import ctypes as C
import itertools

import numpy as np

from . import VisoError, _call, _Handle, _map16, _params, _pose_arg, _struct_arg, load
from .abi import (FIELD_NONE, FIELD_STATE_SURFACE, FIELD_UNKNOWN_IS_SITE, MAP_DEFAULTS, MAP_ENTRY_DTYPE, TSDF_ALIGN_DEFAULTS, TSDF_ALIGN_GRAY_DEFAULTS, TSDF_ALIGN_GRAY_STEP_DTYPE,
                  TSDF_ALIGN_STEP_DTYPE, TSDF_ALIGNMENT_DTYPE, TSDF_ALIGNMENT_GRAY_DTYPE, TSDF_CROSSING_DTYPE, TSDF_DEFAULTS,
                  TSDF_ENTRY_DTYPE, TSDF_FUSE_DEFAULTS, TSDF_GRAY_ENTRY_DTYPE, TSDF_MESH_VERTEX_DTYPE, TSDF_NORMAL_COUNTERS, TSDF_NORMAL_DTYPE,
                  TSDF_NORMAL_GRAY_COUNTERS, TSDF_NORMAL_GRAY_DTYPE, MapCounters, MapParams, TsdfAlignGrayParams, TsdfAlignParams,
                  TsdfCounters, TsdfParams, TsdfRetractReport, VoxelBox, ptr)


def map_params(**params):
    """viso_map_params: viso_map_params_default with the given fields (voxel in metres, min_disp16 in 1/16 px, capacity_log2)
    replaced.  Needs no library: the ranges are checked by viso_map_create (MapParams.ok restates them)."""
    return _params(MapParams, MAP_DEFAULTS, "map_params", params)


def map_entry_centroids(entries, voxel):
    """viso_map_entry_centroid of every entry: float32 [n][3], the mean position of the points fused into each voxel.  Host only."""
    entries = np.ascontiguousarray(entries, dtype=MAP_ENTRY_DTYPE)
    out = np.empty((len(entries), 3), np.float32)
    L = load()
    for i in range(len(entries)):
        _call(L.viso_map_entry_centroid, entries[i:i + 1].ctypes.data, float(voxel), ptr(out[i], C.c_float))
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


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)


def write_map_ply(path, entries, voxel):
    """The entries of VoxelMap.entries as a point cloud file (map_ply_bytes)."""
    _write(path, map_ply_bytes(entries, voxel))


def voxel_box(centre, half_side, voxel):
    """viso_voxel_box_around: (lo, hi), two int32 [3] arrays, the box of the voxels of edge `voxel` that a cube of half-side
    half_side around centre touches: voxel k is inside when lo <= k < hi on every axis (include/viso_hip.h, "Map eviction")."""
    c = np.ascontiguousarray(centre, dtype=np.float64)
    if c.shape != (3,):
        raise ValueError("voxel_box: the centre must have 3 entries")
    b = VoxelBox()
    _call(load().viso_voxel_box_around, ptr(c, C.c_double), float(half_side), float(voxel), C.byref(b))
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
    return _params(TsdfParams, TSDF_DEFAULTS, "tsdf_params", params)


def tsdf_fuse_options(**options):
    """The four fuse options of a TSDF map (include/viso_hip.h, "TSDF fuse options") as a dict in the order of
    viso_tsdf_set_fuse_options' parameters: a new map's (TSDF_FUSE_DEFAULTS) with the given ones replaced: carve_voxels (0: off),
    weight_shift (None or -1: every update weighs 1), weight_max, carve_near in metres.  Needs no library: the ranges are checked
    by viso_tsdf_set_fuse_options."""
    o = dict(TSDF_FUSE_DEFAULTS)
    for k, v in options.items():
        if k not in o:
            raise TypeError(f"tsdf_fuse_options: unknown option {k!r}")
        o[k] = float(v) if k == "carve_near" else -1 if v is None and k == "weight_shift" else int(v)
    return o


def tsdf_align_params(**params):
    """viso_tsdf_align_params: viso_tsdf_align_params_default with the given fields (min_weight, gate_voxels, max_iters, eps_rot in
    rad, eps_trans in metres, min_pixels) replaced.  Needs no library: the ranges are checked by the calls (TsdfAlignParams.ok
    restates them)."""
    return _params(TsdfAlignParams, TSDF_ALIGN_DEFAULTS, "tsdf_align_params", params)


def tsdf_align_gray_params(**params):
    """viso_tsdf_align_gray_params: viso_tsdf_align_gray_params_default with the given fields replaced: those of tsdf_align_params,
    photo_weight (pixels of disparity per gray level) and photo_gate (gray levels).  Needs no library."""
    photo = {k: params.pop(k) for k in tuple(params) if k in TSDF_ALIGN_GRAY_DEFAULTS}
    p = _params(TsdfAlignGrayParams, TSDF_ALIGN_GRAY_DEFAULTS, "tsdf_align_gray_params", photo)
    p.geo = tsdf_align_params(**params)
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
        _call(L.viso_tsdf_crossing_point, crossings[i:i + 1].ctypes.data, float(voxel), ptr(out[i], C.c_float))
    return out


_PLY_XYZW = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("weight", "<u4")]
_PLY_XYZW_HEAD = "property float x\nproperty float y\nproperty float z\nproperty uint weight\n"
_PLY_RGB = [("red", "u1"), ("green", "u1"), ("blue", "u1")]
_PLY_RGB_HEAD = "property uchar red\nproperty uchar green\nproperty uchar blue\n"
_PLY_XYZ, _PLY_W = _PLY_XYZW[:3], _PLY_XYZW[3:]
_PLY_XYZ_HEAD, _PLY_W_HEAD = "property float x\nproperty float y\nproperty float z\n", "property uint weight\n"
_PLY_N = [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
_PLY_N_HEAD = "property float nx\nproperty float ny\nproperty float nz\n"


def _ply_vertices(where, x, y, z, weight, gray, normals=None):
    """(the vertex element's property lines, its records): x, y, z, with normals (float32 [n][3]) nx, ny, nz, then weight and, with
    gray (uint8, one a vertex), red = green = blue."""
    if gray is not None:
        gray = np.asarray(gray)
        if gray.dtype != np.uint8 or gray.shape != (len(x),):
            raise ValueError(f"{where}: gray must be a uint8 array with one value a vertex")
    if normals is not None:
        normals = np.asarray(normals)
        if normals.dtype != np.float32 or normals.shape != (len(x), 3):
            raise ValueError(f"{where}: normals must be a float32 array with three values a vertex")
    v = np.empty(len(x), np.dtype(_PLY_XYZ + (_PLY_N if normals is not None else []) + _PLY_W + (_PLY_RGB if gray is not None else [])))
    v["x"], v["y"], v["z"], v["weight"] = x, y, z, weight
    if normals is not None:
        v["nx"], v["ny"], v["nz"] = normals[:, 0], normals[:, 1], normals[:, 2]
    if gray is not None:
        v["red"] = v["green"] = v["blue"] = gray
    return _PLY_XYZ_HEAD + (_PLY_N_HEAD if normals is not None else "") + _PLY_W_HEAD + (_PLY_RGB_HEAD if gray is not None else ""), v


def _ply_normals(where, normals):
    if normals is None:
        raise ValueError(f"{where}: normals must be a float32 array with three values a vertex")
    return normals


def shade_normals(normals, light=(0.0, 0.0, -1.0)):
    """uint8 [...]: the Lambert shade floor(255 max(0, n . l) + 0.5) of float [...][3] normals (TsdfMap.normals.render, in
    the camera frame, where (0, 0, -1) is a light at the camera) under the direction `light`, which is normalised here.  0 where
    the normal is (0, 0, 0).  Numpy only."""
    n = np.asarray(normals, np.float64)
    l = np.asarray(light, np.float64)
    if n.shape[-1:] != (3,) or l.shape != (3,) or not np.isfinite(l).all() or not l.any():
        raise ValueError("shade_normals: normals must be [...][3] and light three finite numbers, not all zero")
    l = l / np.sqrt((l * l).sum())
    dot = (n[..., 0] * l[0] + n[..., 1] * l[1]) + n[..., 2] * l[2]
    return np.floor(255.0 * np.maximum(0.0, dot) + 0.5).astype(np.uint8)


def _surface_ply(where, crossings, voxel, gray, normals):
    crossings = np.ascontiguousarray(crossings, dtype=TSDF_CROSSING_DTYPE)
    c = tsdf_crossing_points(crossings, voxel)
    props, v = _ply_vertices(where, c[:, 0], c[:, 1], c[:, 2], np.minimum(crossings["wa"], crossings["wb"]), gray, normals)
    head = ("ply\nformat binary_little_endian 1.0\ncomment libviso_amd TSDF surface, voxel %r m\nelement vertex %d\n"
            "%send_header\n" % (float(voxel), len(crossings), props))
    return head.encode("ascii") + v.tobytes()


def surface_ply_bytes(crossings, voxel, gray=None):
    """The bytes of write_surface_ply: a binary little-endian PLY with one vertex per crossing, x, y, z the float32 crossing point
    and weight = min(wa, wb) a uint32, in the crossings' order.  gray (uint8 [n], TsdfMap.vertex_gray of the crossings): red, green
    and blue, all equal to it, follow weight."""
    return _surface_ply("surface_ply_bytes", crossings, voxel, gray, None)


def write_surface_ply(path, crossings, voxel, gray=None):
    """The crossings of TsdfMap.surface as a point cloud file (surface_ply_bytes)."""
    _write(path, surface_ply_bytes(crossings, voxel, gray))


def surface_normals_ply_bytes(crossings, voxel, normals, gray=None):
    """surface_ply_bytes with the crossings' normals (float32 [n][3], TsdfMap.normals.surface): float nx, ny, nz follow x, y, z."""
    return _surface_ply("surface_normals_ply_bytes", crossings, voxel, gray, _ply_normals("surface_normals_ply_bytes", normals))


def write_surface_normals_ply(path, crossings, voxel, normals, gray=None):
    """The crossings of TsdfMap.surface with their normals as a point cloud file (surface_normals_ply_bytes)."""
    _write(path, surface_normals_ply_bytes(crossings, voxel, normals, gray))


def _mesh_ply(where, vertices, triangles, gray, normals):
    vertices = np.ascontiguousarray(vertices, dtype=TSDF_MESH_VERTEX_DTYPE)
    triangles = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
    if len(triangles) and (int(triangles.max()) >= len(vertices) or len(vertices) > 2 ** 31):
        raise ValueError(f"{where}: a triangle refers to a vertex that is not in the list (or is beyond int32)")
    props, v = _ply_vertices(where, vertices["p"][:, 0], vertices["p"][:, 1], vertices["p"][:, 2], vertices["weight"], gray, normals)
    f = np.empty(len(triangles), np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    f["n"], f["v"] = 3, triangles
    head = ("ply\nformat binary_little_endian 1.0\ncomment libviso_amd TSDF mesh\nelement vertex %d\n"
            "%selement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(vertices), props, len(triangles)))
    return head.encode("ascii") + v.tobytes() + f.tobytes()


def mesh_ply_bytes(vertices, triangles, gray=None):
    """The bytes of write_mesh_ply: a binary little-endian PLY; per vertex x, y, z the float32 position and weight a uint32, per
    face a uchar 3 and three int32 vertex indices, both in the order given.  gray (uint8 [n], the third array of
    TsdfMap.mesh(gray=True)): red, green and blue, all equal to it, follow weight."""
    return _mesh_ply("mesh_ply_bytes", vertices, triangles, gray, None)


def write_mesh_ply(path, vertices, triangles, gray=None):
    """The mesh of TsdfMap.mesh as a PLY file (mesh_ply_bytes)."""
    _write(path, mesh_ply_bytes(vertices, triangles, gray))


def mesh_normals_ply_bytes(vertices, triangles, normals, gray=None):
    """mesh_ply_bytes with the vertices' normals (float32 [n][3], the last array of TsdfMap.normals.mesh): float nx, ny, nz follow
    x, y, z, so that a viewer shades the mesh smoothly."""
    return _mesh_ply("mesh_normals_ply_bytes", vertices, triangles, gray, _ply_normals("mesh_normals_ply_bytes", normals))


def write_mesh_normals_ply(path, vertices, triangles, normals, gray=None):
    """The mesh of TsdfMap.normals.mesh as a PLY file (mesh_normals_ply_bytes)."""
    _write(path, mesh_normals_ply_bytes(vertices, triangles, normals, gray))


def _vertex_list(vertices):
    """The (k, dir) list of a per-vertex call: mesh vertices as they are, crossings as dir = 1 << axis."""
    if getattr(vertices, "dtype", None) == TSDF_CROSSING_DTYPE:
        c = vertices
        vertices = np.zeros(len(c), TSDF_MESH_VERTEX_DTYPE)
        vertices["k"], vertices["dir"] = c["k"], np.left_shift(1, c["axis"])
    return np.ascontiguousarray(vertices, dtype=TSDF_MESH_VERTEX_DTYPE)


def _reported(fn, *args):
    """fn(*args, report) of a retract or a move (include/viso_hip.h, "TSDF retract"): the report as a dict of n_points, n_updates,
    n_missing, n_underflow, n_inconsistent, n_freed.  A refusal raises the library's error with the dict as its .report."""
    rep = TsdfRetractReport()
    try:
        _call(fn, *args, rep.words())
    except VisoError as e:
        e.report = rep.as_dict()
        raise
    return rep.as_dict()


class _TableMap(_Handle):
    """What VoxelMap and TsdfMap share: a handle of one of the two kinds of hash tables of voxels (csrc/voxel_host.h).  A subclass
    sets _prefix (the C functions are _prefix + name), _Params and _params (the parameter struct and its factory), _ENTRY_DTYPE and
    _Counters."""

    def __init__(self, ctx=None, params=None, **kw):
        self.L = load()
        params = _struct_arg(type(self).__name__, self._Params, type(self)._params, params, kw)
        self.ctx, self._p, self.voxel = ctx, params, float(params.voxel)
        h = C.c_void_p()
        _call(self._c("create"), ctx.h if ctx is not None else None, C.byref(params), C.byref(h))
        self._own(h.value)

    def _c(self, name):
        return getattr(self.L, self._prefix + name)

    def fuse(self, d16, param, pose=None):
        """viso_map_fuse / viso_tsdf_fuse: one host int16 map with the calibration of param (f, cu, cv, base) and an optional 4 x 4
        pose."""
        where = type(self).__name__ + ".fuse"
        d16 = _map16(where, d16)
        T, Tp = _pose_arg(where, pose, square=True)
        _call(self._c("fuse"), self.h, ptr(d16, C.c_int16), d16.shape[0], d16.shape[1], C.byref(param), Tp)

    def add_entries(self, entries):
        """viso_map_add_entries / viso_tsdf_add_entries: the entries of another map with the same voxel (a TSDF map: and truncation),
        or of a saved one, added to this one."""
        entries = np.ascontiguousarray(entries, dtype=self._ENTRY_DTYPE)
        _call(self._c("add_entries"), self.h, entries.ctypes.data, len(entries))

    def _count(self, count_name, threshold):
        n = C.c_size_t()
        _call(self._c(count_name), self.h, int(threshold), C.byref(n))
        return n

    def _list(self, count_name, get_name, dtype, threshold):
        n = self._count(count_name, threshold)
        out = np.zeros(n.value, dtype)
        _call(self._c(get_name), self.h, int(threshold), out.ctypes.data, len(out), C.byref(n))
        return out[:n.value]

    def _evict_dtype(self):
        return self._ENTRY_DTYPE

    def evict_count(self, box):
        """viso_map_evict_count / viso_tsdf_evict_count: the number of voxels outside box = (lo, hi); reads only."""
        n = C.c_size_t()
        _call(self._c("evict_count"), self.h, C.byref(_box_arg(type(self).__name__ + ".evict_count", box)), C.byref(n))
        return n.value

    def evict(self, box, discard=False):
        """viso_map_evict / viso_tsdf_evict / viso_tsdf_evict_gray: every voxel outside box = (lo, hi) (voxel_box makes one around
        a point) leaves the map, on the device, and its slot is free again.  Returns the evicted voxels as an array of the map's
        own entry dtype (a gray map's: TSDF_GRAY_ENTRY_DTYPE), sorted by key; merge_entries of them and of what the map holds
        later is the map that was never evicted.  discard=True: they are dropped on the device, and their number comes back."""
        b = _box_arg(type(self).__name__ + ".evict", box)
        dtype = self._evict_dtype()
        evict = self._c("evict_gray" if dtype == TSDF_GRAY_ENTRY_DTYPE else "evict")
        n = C.c_size_t()
        if discard:
            _call(evict, self.h, C.byref(b), None, 0, C.byref(n))
            return n.value
        _call(self._c("evict_count"), self.h, C.byref(b), C.byref(n))
        out = np.zeros(n.value, dtype)
        _call(evict, self.h, C.byref(b), out.ctypes.data, len(out), C.byref(n))
        return out[:n.value]

    def stats(self):
        """viso_map_stats / viso_tsdf_stats as a dict of the counters' fields."""
        c = self._Counters()
        _call(self._c("stats"), self.h, C.byref(c))
        return {name: int(getattr(c, name)) for name, _ in self._Counters._fields_}

    def clear(self):
        _call(self._c("clear"), self.h)


class VoxelMap(_TableMap):
    """viso_map: a persistent voxel map on the device that dense disparity maps and their poses are fused into (opt-in, not in the
    reference; the definition of include/viso_hip.h).  ctx: a Context, or None for the default one.  With a trajectory:

        poses, valid = hostmath.chain_poses(tr, ok)      # poses[k + 1] places frame valid[k] in frame 0's coordinates
        vmap = VoxelMap(ctx, voxel=0.2)
        for k, t in enumerate(valid):
            batch.fuse_disparities(vmap, poses[k + 1][None], t0=t, t1=t + 1)
        write_map_ply("scene.ply", vmap.entries(min_count=2), vmap.voxel)
    """
    _prefix, _destroy, _Params, _params, _ENTRY_DTYPE, _Counters = ("viso_map_", "viso_map_destroy", MapParams, map_params,
                                                                    MAP_ENTRY_DTYPE, MapCounters)

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

    carve_voxels=0, weight_shift=None, weight_max=255, carve_near=0.0: the map's fuse options (include/viso_hip.h, "TSDF fuse
    options"; the property fuse_options), which every way of fusing into it obeys, Batch.fuse_tsdf included.  carve_voxels=C: a pixel's ray
    also updates the C voxels in front of its band, so surfaces that later frames look through go away; weight_shift=S: an update
    weighs min(max(disp16^2 >> S, 1), weight_max) and not 1, so min_weight then compares sums of such weights.
    """
    _prefix, _destroy, _Params, _params, _ENTRY_DTYPE, _Counters = ("viso_tsdf_", "viso_tsdf_destroy", TsdfParams, tsdf_params,
                                                                    TSDF_ENTRY_DTYPE, TsdfCounters)

    def __init__(self, ctx=None, params=None, gray=False, **kw):
        self.gray = bool(gray)
        options = {k: kw.pop(k) for k in tuple(kw) if k in TSDF_FUSE_DEFAULTS}
        super().__init__(ctx, params, **kw)
        self.trunc_voxels = int(self._p.trunc_voxels)
        if options:
            try:
                self.fuse_options = options
            except Exception:
                self.close()
                raise

    @property
    def fuse_options(self):
        """The map's fuse options as a dict: carve_voxels, weight_shift (None: off), weight_max, carve_near
        (viso_tsdf_get_fuse_options).  Assigning a dict of some of them (`tsdf.fuse_options = dict(carve_voxels=28)`; the ones not
        given: a new map's, not the map's current values) sets them for every later fuse into this map
        (viso_tsdf_set_fuse_options); they persist across clear().  Bad values raise and leave the map's as they were.  A property
        and its setter, not two methods."""
        c, s, m, n = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_double()
        _call(self.L.viso_tsdf_get_fuse_options, self.h, C.byref(c), C.byref(s), C.byref(m), C.byref(n))
        return dict(carve_voxels=c.value, weight_shift=None if s.value < 0 else s.value, weight_max=m.value, carve_near=n.value)

    @fuse_options.setter
    def fuse_options(self, options):
        o = tsdf_fuse_options(**options)
        _call(self.L.viso_tsdf_set_fuse_options, self.h, o["carve_voxels"], o["weight_shift"], o["weight_max"], o["carve_near"])

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
        d16, image = _map16("TsdfMap.fuse", d16), np.ascontiguousarray(image)
        if image.dtype != np.uint8 or image.shape != d16.shape:
            raise ValueError("TsdfMap.fuse: the image must be a 2-D uint8 array of the map's shape")
        T, Tp = _pose_arg("TsdfMap.fuse", pose, square=True)
        _call(self.L.viso_tsdf_fuse_gray, self.h, ptr(d16, C.c_int16), ptr(image, C.c_uint8), d16.shape[0], d16.shape[1],
              C.byref(param), Tp)

    def add_entries(self, entries):
        """viso_tsdf_add_entries, or for a TSDF_GRAY_ENTRY_DTYPE array viso_tsdf_add_gray_entries: the entries of another map of
        the same kind, voxel and truncation, or of a saved one, added to this one."""
        if getattr(entries, "dtype", None) != TSDF_GRAY_ENTRY_DTYPE:
            return super().add_entries(entries)
        entries = np.ascontiguousarray(entries)
        _call(self.L.viso_tsdf_add_gray_entries, self.h, entries.ctypes.data, len(entries))

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
        vertices = _vertex_list(vertices)
        g, n_missing = np.zeros(len(vertices), np.uint8), C.c_size_t()
        _call(self.L.viso_tsdf_vertex_gray, self.h, vertices.ctypes.data, len(vertices), ptr(g, C.c_uint8), C.byref(n_missing))
        return (g, n_missing.value) if missing else g

    @property
    def retract(self):
        """viso_tsdf_retract / viso_tsdf_retract_gray (include/viso_hip.h, "TSDF retract"), called as
        `tsdf.retract(d16, param, pose=None, image=None)` with the arguments the frame was fused with: its updates are taken out of
        the map again, bit for bit, and the voxels whose weight returns to zero leave the table.  Returns the report as a dict
        (n_points, n_updates, n_missing, n_underflow, n_inconsistent, n_freed).  A frame that is not in the map as given is refused:
        the library's error is raised with the report as its .report, and the map is unchanged.  A property that hands out the
        call, like distance_field."""
        return _RetractCall(self)

    @property
    def move(self):
        """viso_tsdf_move / viso_tsdf_move_gray, called as `tsdf.move(d16, param, old_pose, new_pose, image=None)`: retract at
        old_pose and, if that is not refused, fuse at new_pose, under one hold on the map.  Returns the retract's report."""
        return _MoveCall(self)

    @property
    def normals(self):
        """The surface normals of this map (include/viso_hip.h, "TSDF normals"): a TsdfNormals, whose vertices, surface, mesh and
        render give a unit normal for every vertex, crossing and rendered hit.  A plain or a gray map."""
        return TsdfNormals(self)

    @property
    def distance_field(self):
        """viso_tsdf_distance_field (include/viso_hip.h, "TSDF distance field"), called as
        `tsdf.distance_field(box, min_weight=2, unknown_is_site=False)`: a DistanceField over box = (lo, hi) (voxel_box makes one
        around a point; 1 .. 512 voxels an axis), for every voxel of it the exact squared distance in voxels to the nearest
        surface voxel of the box at min_weight; unknown_is_site=True: to the nearest surface or unknown voxel, the conservative field
        for planning.  Surface beyond the box does not exist for the call: pad the box by the clearance that matters.  Reads the
        map only; a plain or a gray map.  A property that hands out the call, not a method."""
        return _DistanceFieldCall(self)

    @property
    def travel_field(self):
        """viso_tsdf_travel_field (include/viso_hip.h, "TSDF travel field"), called as
        `tsdf.travel_field(box, goals, clearance=0.0, min_weight=2, unknown_is_site=True)`: a TravelField over box = (lo, hi), for
        every voxel of it the cost of the cheapest way to a goal for a body that keeps `clearance` metres from the surface, and the
        paths that follow from it (_TravelFieldCall has the arguments).  Reads the map only; a plain or a gray map.  A property
        that hands out the call, like distance_field."""
        return _TravelFieldCall(self)

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
        _call(self.L.viso_tsdf_mesh_count, self.h, int(min_weight), C.byref(nv), C.byref(nt))
        v, tri = np.zeros(nv.value, TSDF_MESH_VERTEX_DTYPE), np.zeros((nt.value, 3), np.uint32)
        _call(self.L.viso_tsdf_mesh, self.h, int(min_weight), v.ctypes.data, len(v), tri.ctypes.data, len(tri), C.byref(nv), C.byref(nt))
        v, tri = v[:nv.value], tri[:nt.value]
        return (v, tri, self.vertex_gray(v)) if gray else (v, tri)

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
        d16 = _map16("TsdfMap.linearize", d16)
        T, Tp = _pose_arg("TsdfMap.linearize", pose, square=True)
        if image is not None:
            image = self._align_image("TsdfMap.linearize", image, d16)
            p, out = tsdf_align_gray_params(**params), np.zeros(1, TSDF_NORMAL_GRAY_DTYPE)
            _call(self.L.viso_tsdf_linearize_gray, self.h, C.byref(p), ptr(d16, C.c_int16), ptr(image, C.c_uint8), d16.shape[0],
                  d16.shape[1], C.byref(param), Tp, out.ctypes.data)
            return tsdf_normal_gray_matrix(out[0])
        p, out = tsdf_align_params(**params), np.zeros(1, TSDF_NORMAL_DTYPE)
        _call(self.L.viso_tsdf_linearize, self.h, C.byref(p), ptr(d16, C.c_int16), d16.shape[0], d16.shape[1], C.byref(param), Tp,
              out.ctypes.data)
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
        d16 = _map16("TsdfMap.align", d16)
        T, Tp = _pose_arg("TsdfMap.align", pose, square=True)
        if image is not None:
            image = self._align_image("TsdfMap.align", image, d16)
            p, rec, step_dtype = tsdf_align_gray_params(**params), np.zeros(1, TSDF_ALIGNMENT_GRAY_DTYPE), TSDF_ALIGN_GRAY_STEP_DTYPE
            fn, args, max_iters = self.L.viso_tsdf_align_gray, (ptr(d16, C.c_int16), ptr(image, C.c_uint8)), p.geo.max_iters
        else:
            p, rec, step_dtype = tsdf_align_params(**params), np.zeros(1, TSDF_ALIGNMENT_DTYPE), TSDF_ALIGN_STEP_DTYPE
            fn, args, max_iters = self.L.viso_tsdf_align, (ptr(d16, C.c_int16),), p.max_iters
        steps = np.zeros(max_iters + 1 if trace and 1 <= max_iters <= 50 else 0, step_dtype)
        _call(fn, self.h, C.byref(p), *args, d16.shape[0], d16.shape[1], C.byref(param), Tp, rec.ctypes.data,
              steps.ctypes.data if len(steps) else None, len(steps))
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
        return self._render(param, shape, poses, max_depth, min_weight, weights, gray, False)

    def _render(self, param, shape, poses, max_depth, min_weight, weights, gray, normals):
        """render, and with normals (TsdfNormals.render) viso_tsdf_render_normals: the tuple ends with float32 [..][rows][cols][3]."""
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
        nrm = np.empty((n, rows, cols, 3), np.float32) if normals else None
        if gray:
            _call(self.L.viso_tsdf_render_gray, *args, ptr(g, C.c_uint8))
        if normals:
            _call(self.L.viso_tsdf_render_normals, *args, ptr(nrm, C.c_float))
        if not gray and not normals:
            _call(self.L.viso_tsdf_render, *args)
        if T is None or T.ndim == 2:
            d, w, g, nrm = d[0], (w[0] if weights else None), (g[0] if gray else None), (nrm[0] if normals else None)
        out = (d,) + ((w,) if weights else ()) + ((g,) if gray else ()) + ((nrm,) if normals else ())
        return out if len(out) > 1 else d


def _retract(t, where, name, d16, param, poses, image):
    """viso_tsdf_<name>, or on a gray map viso_tsdf_<name>_gray, of one host map at `poses` (one for a retract, old and new for a move)."""
    if (image is not None) != t.gray:
        raise ValueError(f"{where}: a gray map's frame comes with its image, a plain one's without")
    d16 = _map16(where, d16)
    T = [_pose_arg(where, p, square=True) for p in poses]   # (the list keeps the arrays alive over the call)
    args = (ptr(d16, C.c_int16),)
    if t.gray:
        image = np.ascontiguousarray(image)
        if image.dtype != np.uint8 or image.shape != d16.shape:
            raise ValueError(f"{where}: the image must be a 2-D uint8 array of the map's shape")
        args += (ptr(image, C.c_uint8),)
    fn = getattr(t.L, "viso_tsdf_" + name + ("_gray" if t.gray else ""))
    return _reported(fn, t.h, *args, d16.shape[0], d16.shape[1], C.byref(param), *(Tp for _, Tp in T))


class _RetractCall:
    """What TsdfMap.retract hands out: the call on that map."""

    def __init__(self, tsdf):
        self.tsdf = tsdf

    def __call__(self, d16, param, pose=None, image=None):
        return _retract(self.tsdf, "TsdfMap.retract", "retract", d16, param, (pose,), image)


class _MoveCall:
    """What TsdfMap.move hands out: the call on that map."""

    def __init__(self, tsdf):
        self.tsdf = tsdf

    def __call__(self, d16, param, old_pose, new_pose, image=None):
        return _retract(self.tsdf, "TsdfMap.move", "move", d16, param, (old_pose, new_pose), image)


class DistanceField:
    """TsdfMap.distance_field: the distance field of a TSDF map's surface over a box of voxels (include/viso_hip.h, "TSDF distance
    field").  sq: uint32 (n0, n1, n2), the squared distance of cell i (the voxel box[0] + i) to the nearest site in voxels, FIELD_NONE
    everywhere when the box has no site; state: uint8 of the same shape, 0 unknown, 1 in front of the surface, 2 behind it, plus
    FIELD_STATE_SURFACE on surface voxels; box = (lo, hi) as int32 [3] arrays; voxel in metres; n_sites."""

    def __init__(self, sq, state, box, voxel, n_sites):
        self.sq, self.state, self.voxel, self.n_sites = sq, state, float(voxel), int(n_sites)
        self.box = (np.array(box[0], np.int32), np.array(box[1], np.int32))

    def metres(self):
        """float32 (n0, n1, n2): sqrt(sq) * voxel computed in double, inf where there is no site."""
        d = np.sqrt(self.sq.astype(np.float64)) * self.voxel
        return np.where(self.sq == FIELD_NONE, np.inf, d).astype(np.float32)

    def signed_metres(self):
        """metres(), negated where the state is behind the surface."""
        d = self.metres()
        return np.where((self.state & 3) == 2, -d, d)

    def at(self, points):
        """(sq, outside) of float [n][3] points in metres: sq of the cell floor(p / voxel) - lo that holds each point (uint32 [n],
        FIELD_NONE for a point outside the box), and the bool [n] mask of the points outside the box (not finite ones included)."""
        p = np.asarray(points, np.float64)
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError("DistanceField.at: points must be [n][3]")
        with np.errstate(invalid="ignore"):
            cell = np.floor(p / self.voxel) - self.box[0].astype(np.float64)
            outside = ~((cell >= 0) & (cell < np.asarray(self.sq.shape, np.float64))).all(axis=1)   # a NaN is outside
        i = np.where(outside[:, None], 0, cell).astype(np.int64)
        return np.where(outside, np.uint32(FIELD_NONE), self.sq[i[:, 0], i[:, 1], i[:, 2]]).astype(np.uint32), outside


class _DistanceFieldCall:
    """What TsdfMap.distance_field hands out: the call on that map."""

    def __init__(self, tsdf):
        self.tsdf = tsdf

    def __call__(self, box, min_weight=2, unknown_is_site=False):
        t = self.tsdf
        b = _box_arg("TsdfMap.distance_field", box)
        lo, hi = np.array(b.lo, np.int64), np.array(b.hi, np.int64)
        n = hi - lo
        if (n < 1).any() or (n > 512).any():
            raise ValueError("TsdfMap.distance_field: the box must have 1 .. 512 voxels on every axis")
        sq, state, n_sites = np.empty(tuple(n), np.uint32), np.empty(tuple(n), np.uint8), C.c_size_t()
        _call(t.L.viso_tsdf_distance_field, t.h, int(min_weight), C.byref(b), FIELD_UNKNOWN_IS_SITE if unknown_is_site else 0,
              ptr(sq, C.c_uint32), ptr(state, C.c_uint8), sq.size, C.byref(n_sites))
        return DistanceField(sq, state, (lo, hi), t.voxel, n_sites.value)


class _TravelFieldCall:
    """What TsdfMap.travel_field hands out: the call on that map."""

    def __init__(self, tsdf):
        self.tsdf = tsdf

    def __call__(self, box, goals=None, clearance=0.0, min_weight=2, unknown_is_site=True, clearance_sq=None, goals_m=None):
        """viso_tsdf_travel_field (include/viso_hip.h, "TSDF travel field"): a TravelField over box = (lo, hi), for every voxel of it
        the cost in thirds of a voxel of the cheapest way, by <3,4,5> chamfer moves through free cells, to one of the goals.  A
        cell is free when it is not behind the surface, is no site of the distance field at min_weight, and its nearest site is at
        least `clearance` metres away (travel_clearance_sq has the rounding; clearance_sq= gives the squared clearance in voxels
        directly).  unknown_is_site=True, the default here: what was never seen is an obstacle, the conservative field; False: the
        optimistic one.  goals: voxel indices [n][3] (or one [3]); goals_m= instead: points in metres, each the voxel
        floor(p / voxel) that holds it.  Goals outside the box or in cells that are not free are skipped.  Reads the map only."""
        where, t = "TsdfMap.travel_field", self.tsdf
        b = _box_arg(where, box)
        lo, hi = np.array(b.lo, np.int64), np.array(b.hi, np.int64)
        n = hi - lo
        if (n < 1).any() or (n > 512).any():
            raise ValueError(f"{where}: the box must have 1 .. 512 voxels on every axis")
        if (goals is None) == (goals_m is None):
            raise ValueError(f"{where}: either goals (voxel indices) or goals_m (points in metres)")
        if goals_m is not None:
            p = np.atleast_2d(np.asarray(goals_m, np.float64))
            if p.ndim != 2 or p.shape[1] != 3 or not np.isfinite(p).all():
                raise ValueError(f"{where}: goals_m must be finite points [n][3]")
            g = np.floor(p / t.voxel)
        else:
            g = np.atleast_2d(np.asarray(goals))
            if g.ndim != 2 or g.shape[1] != 3 or not np.issubdtype(g.dtype, np.integer):
                raise ValueError(f"{where}: goals must be voxel indices [n][3]")
        i32 = np.iinfo(np.int32)
        if len(g) and (g.min() < i32.min or g.max() > i32.max):
            raise ValueError(f"{where}: the goals must be int32 voxel indices")
        g = np.ascontiguousarray(g, dtype=np.int32)
        if clearance_sq is None:
            clearance_sq = travel_clearance_sq(clearance, t.voxel)
        elif clearance != 0.0:
            raise ValueError(f"{where}: either clearance or clearance_sq")
        if not 0 <= int(clearance_sq) <= FIELD_NONE:
            raise ValueError(f"{where}: clearance_sq must be a uint32 value")
        shape = tuple(int(v) for v in n)
        cost, sq, state = np.empty(shape, np.uint32), np.empty(shape, np.uint32), np.empty(shape, np.uint8)
        n_used, n_reached, n_rounds = C.c_size_t(), C.c_size_t(), C.c_size_t()
        flags = FIELD_UNKNOWN_IS_SITE if unknown_is_site else 0
        _call(t.L.viso_tsdf_travel_field, t.h, int(min_weight), C.byref(b), flags, int(clearance_sq), ptr(g, C.c_int32), len(g),
              ptr(cost, C.c_uint32), ptr(sq, C.c_uint32), ptr(state, C.c_uint8), cost.size, C.byref(n_used), C.byref(n_reached),
              C.byref(n_rounds))
        site = (state & FIELD_STATE_SURFACE) != 0
        if unknown_is_site:
            site |= (state & 3) == 0
        n_sites = int(site.sum())        # (the sites are the cells the states say: rule 5 of the distance field)
        return TravelField(cost, DistanceField(sq, state, (lo, hi), t.voxel, n_sites), (lo, hi), t.voxel, clearance_sq,
                           n_used.value, n_reached.value, n_rounds.value)


# the 26 moves of a travel field in the order in which TravelField.path tries them, and what each costs
TRAVEL_MOVES = np.array([e for e in itertools.product((-1, 0, 1), repeat=3) if e != (0, 0, 0)], np.int64)
TRAVEL_MOVE_COSTS = 2 + (TRAVEL_MOVES != 0).sum(axis=1)


def travel_clearance_sq(clearance, voxel):
    """clearance_sq of a clearance in metres: the smallest integer n with n voxel^2 >= clearance^2, so that sq >= n says exactly
    that the nearest site is at least the clearance away.  Both doubles are taken at their exact values and the rest is integer
    arithmetic: with clearance = p / q and voxel = r / s, n = ceil(p^2 s^2 / (q^2 r^2)).  No rounding of a quotient or a square
    can let a body through a gap that the two numbers say it does not fit; a clearance a hair above k voxels gives k^2 + 1."""
    clearance, voxel = float(clearance), float(voxel)
    if not (np.isfinite(clearance) and clearance >= 0 and np.isfinite(voxel) and voxel > 0):
        raise ValueError("travel_clearance_sq: the clearance must be finite and >= 0, the voxel finite and > 0")
    (p, q), (r, s) = clearance.as_integer_ratio(), voxel.as_integer_ratio()
    num, den = p * p * s * s, q * q * r * r
    n = -(-num // den)        # the ceiling of num / den
    if n >= FIELD_NONE:
        raise ValueError("travel_clearance_sq: the clearance is beyond every box (clearance_sq must stay below FIELD_NONE)")
    return n


class TravelField:
    """TsdfMap.travel_field: the travel field of a TSDF map over a box of voxels (include/viso_hip.h, "TSDF travel field").  cost:
    uint32 (n0, n1, n2), the cost of the cheapest sequence of moves from cell i (the voxel box[0] + i) to a used goal in thirds of
    a voxel, FIELD_NONE where the cell is not free or no goal is reached; field: the DistanceField of the same call; box = (lo, hi)
    as int32 [3] arrays; voxel in metres; clearance_sq; n_goals_used, n_reached, rounds."""

    def __init__(self, cost, field, box, voxel, clearance_sq, n_goals_used, n_reached, rounds):
        self.cost, self.field, self.voxel, self.clearance_sq = cost, field, float(voxel), int(clearance_sq)
        self.n_goals_used, self.n_reached, self.rounds = int(n_goals_used), int(n_reached), int(rounds)
        self.box = (np.array(box[0], np.int32), np.array(box[1], np.int32))

    def metres(self):
        """float32 (n0, n1, n2): cost / 3 * voxel computed in double, inf where the cost is FIELD_NONE.  Between 0.943 and 1.106
        times the Euclidean length where nothing is in the way."""
        d = self.cost.astype(np.float64) / 3.0 * self.voxel
        return np.where(self.cost == FIELD_NONE, np.inf, d).astype(np.float32)

    def at(self, points):
        """(cost, outside) of float [n][3] points in metres: the cost of the cell floor(p / voxel) - lo that holds each point
        (uint32 [n], FIELD_NONE for a point outside the box), and the bool [n] mask of the points outside the box (not finite
        ones included): DistanceField.at for the costs."""
        return DistanceField(self.cost, None, self.box, self.voxel, 0).at(points)

    def path(self, start):
        """The way from the voxel `start` (absolute indices [3]) to a goal, as the int32 [m][3] array of the voxels it visits, start
        and goal included; None when start is outside the box or has no finite cost.  From a cell c the path steps to the first
        neighbour n inside the box with cost[n] + w == cost[c], w the move's 3, 4 or 5, first in the order of
        itertools.product((-1, 0, 1), repeat=3) without (0, 0, 0), until the cost is 0.  Runs on the host."""
        k = np.asarray(start)
        if k.shape != (3,) or not np.issubdtype(k.dtype, np.integer):
            raise ValueError("TravelField.path: start must be three voxel indices")
        lo, shape = self.box[0].astype(np.int64), np.asarray(self.cost.shape, np.int64)
        c = k.astype(np.int64) - lo
        if ((c < 0) | (c >= shape)).any() or self.cost[tuple(c)] == FIELD_NONE:
            return None
        cells = [c]
        while self.cost[tuple(c)] != 0:
            here = int(self.cost[tuple(c)])
            n = c + TRAVEL_MOVES
            inside = ((n >= 0) & (n < shape)).all(axis=1)
            there = np.where(inside, self.cost[tuple(np.where(inside[:, None], n, 0).T)].astype(np.int64), -1)
            down = np.flatnonzero(inside & (there != FIELD_NONE) & (there + TRAVEL_MOVE_COSTS == here))
            if not len(down):
                raise ValueError("TravelField.path: the costs are not those of a travel field (no neighbour leads on)")
            c = n[down[0]]
            cells.append(c)
        return (np.array(cells, np.int64) + lo).astype(np.int32)

    def path_metres(self, start):
        """path(start) as float64 [m][3] points in metres, the centres (k + 0.5) voxel of its voxels; None where path gives None."""
        p = self.path(start)
        return None if p is None else (p.astype(np.float64) + 0.5) * self.voxel


class TsdfNormals:
    """TsdfMap.normals: which way the surface of a TSDF map faces (include/viso_hip.h, "TSDF normals").  A normal is the gradient of
    the averaged signed distance over a voxel's six neighbours, interpolated between the two voxels of the edge on which the surface
    point lies: a unit float32 vector towards the cameras that saw the surface, (0, 0, 0) where there is none (an end of the edge
    that is not usable, ends of one sign, or an end without a neighbour on some axis, as along the rim of the data).  The calls read
    weight and sum only, of a plain or a gray map, and change nothing in it."""

    def __init__(self, tsdf):
        self.tsdf = tsdf

    def vertices(self, vertices, min_weight=1, missing=False):
        """viso_tsdf_vertex_normals: float32 [n][3], the normal in the world frame of every vertex of TsdfMap.mesh (a
        TSDF_MESH_VERTEX_DTYPE array, of which k and dir are read) or of every crossing of TsdfMap.surface (a TSDF_CROSSING_DTYPE
        array: dir = 1 << axis), over the voxels of at least min_weight updates.  missing=True: a tuple with the number of
        vertices without a normal."""
        t = self.tsdf
        vertices = _vertex_list(vertices)
        nrm, n_missing = np.zeros((len(vertices), 3), np.float32), C.c_size_t()
        _call(t.L.viso_tsdf_vertex_normals, t.h, int(min_weight), vertices.ctypes.data, len(vertices), ptr(nrm, C.c_float), C.byref(n_missing))
        return (nrm, n_missing.value) if missing else nrm

    def surface(self, min_weight=1):
        """float32 [n][3]: the normals of the crossings of TsdfMap.surface(min_weight), at the same min_weight, in their order."""
        return self.vertices(self.tsdf.surface(min_weight), min_weight)

    def mesh(self, min_weight=1, gray=False):
        """TsdfMap.mesh(min_weight, gray) with the tuple ending in the float32 [n][3] normals of its vertices, at the same
        min_weight: (vertices, triangles, n), or (vertices, triangles, g, n) of a gray map."""
        out = self.tsdf.mesh(min_weight, gray)
        return out + (self.vertices(out[0], min_weight),)

    def render(self, param, shape, poses=None, max_depth=40.0, min_weight=2, weights=False, gray=False):
        """viso_tsdf_render_normals: TsdfMap.render with the same arguments, its tuple ending in the float32 array of the maps' shape
        with a last axis of 3: the normal of every hit in the view's camera frame ((0, 0, 0): none), pixel for pixel the points of
        disparity_to_points of the rendered map.  The map and the weights are TsdfMap.render's, bit for bit.  gray=True (a gray
        map): the intensity comes from a second call on the same table."""
        return self.tsdf._render(param, shape, poses, max_depth, min_weight, weights, gray, True)
