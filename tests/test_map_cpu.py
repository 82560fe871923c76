"""The voxel map of include/viso_hip.h without a device: the two numpy restatements (tests/map_ref.py) against each other, known
answers, additivity, the struct layouts, the argument checks of the C ABI, the centroid, the tool's readers, the PLY bytes, and
the kernels' resource usage."""
import ctypes as C
import struct
import zlib

import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map, hostmath
from libviso_amd.abi import MAP_DEFAULTS, MAP_ENTRY_DTYPE, MapCounters, MapParams, Param

import map_ref as M
from estimator_util import kernel_resources
from test_speckle_cpu import random_map

INV = M.INVALID
POSE = np.linalg.inv(hostmath.tr2mat([0.013, -0.021, 0.007, 0.31, -0.12, 1.47]))


def _param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)


def _same(a, b):
    return a.dtype == b.dtype == M.ENTRY and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("seed", range(4))
def test_vectorised_equals_loop(seed):
    rng = np.random.default_rng(seed)
    rows, cols = int(rng.integers(1, 14)), int(rng.integers(1, 40))
    frames = [(random_map(rng, rows, cols, spread=2100, invalid=0.2), pose) for pose in (None, np.eye(4), POSE)]
    prm = _param()
    for voxel in (0.05, 0.2, 1000.0):
        for md in (1, 160):
            a, sa = M.fuse(frames, prm, voxel, md)
            b, sb = M.fuse_loop(frames, prm, voxel, md)
            assert _same(a, b) and sa == sb and sa["n_out_of_range"] == 0 and sa["n_dropped"] == 0
            assert int(a["count"].sum()) == sa["n_points"] and (np.diff(M.keys_of(a["k"])) > 0).all()
            assert _same(M.fuse(frames, prm, voxel, md, min_count=2)[0], a[a["count"] >= 2])


def _one_pixel(x, y, d16, prm, voxel, pose=None, rows=4, cols=6):
    m = np.full((rows, cols), INV, np.int16)
    m[y, x] = d16
    return M.fuse([(m, pose)], prm, voxel, 1)


def test_known_answers():
    # calibration chosen so that the point is exact: base 1, cu = cv = 0, f = 2, d = 1 px -> P = (x, y, 2)
    prm = Param.default(base=1.0, f=2.0, cu=0.0, cv=0.0)
    e, st = _one_pixel(3, 1, 16, prm, 1.0)
    # s = 1 / 1024: g = (3072, 1024, 2048): on the faces of voxels 3, 1, 2, which own their lower face: offsets 0
    assert len(e) == 1 and e["k"][0].tolist() == [3, 1, 2] and e["count"][0] == 1 and e["sum"][0].tolist() == [0, 0, 0]
    assert st == dict(n_points=1, n_out_of_range=0, n_occupied=1, n_dropped=0)
    assert np.array_equal(M.centroids(e, 1.0), np.array([[3, 1, 2]], np.float32) + np.float32(0.5 / 1024))
    # a computed cell: voxel 0.4, P = (3, 1, 2) -> g = floor(P * 2560) = (7680, 2560, 5120) -> k = (7, 2, 5), o = (512, 512, 0)
    e, _ = _one_pixel(3, 1, 16, prm, 0.4)
    g = [int(np.floor(np.float64(v) / (np.float64(0.4) / 1024.0))) for v in (3, 1, 2)]
    assert e["k"][0].tolist() == [v >> 10 for v in g] and e["sum"][0].tolist() == [v & 1023 for v in g]
    assert e["k"][0].tolist() == [7, 2, 5]
    # negative coordinates: floor, not truncation.  cu = 4.5 puts x = 3 at X = -1.5 -> g = -1536 -> k = -2, o = 512
    neg = Param.default(base=1.0, f=2.0, cu=4.5, cv=0.0)
    e, _ = _one_pixel(3, 0, 16, neg, 1.0)
    assert e["k"][0].tolist() == [-2, 0, 2] and e["sum"][0].tolist() == [512, 0, 0]
    assert np.array_equal(M.centroids(e, 1.0)[0], np.float32([-1.5 + 0.5 / 1024, 0.5 / 1024, 2 + 0.5 / 1024]))
    # a translation by a hair below zero: g = -1, the last offset of voxel -1
    T = np.eye(4); T[1, 3] = -1e-9
    e, _ = _one_pixel(3, 0, 16, prm, 1.0, pose=T)
    assert e["k"][0].tolist() == [3, -1, 2] and e["sum"][0].tolist() == [0, 1023, 0]
    # the range: |g| = 2^30 - 1 is kept, 2^30 dropped.  voxel 1024 -> s = 1, g = floor(P)
    for tz, kept in ((float(M.RANGE - 1 - 2), True), (float(M.RANGE - 2), False), (-float(M.RANGE - 1 + 2), True), (-float(M.RANGE + 3), False)):
        T = np.eye(4); T[2, 3] = tz          # Z = 2 + tz
        e, st = _one_pixel(3, 1, 16, prm, 1024.0, pose=T)
        assert (len(e) == 1) == kept and st["n_out_of_range"] == (0 if kept else 1) and st["n_points"] == 1, tz
        if kept:
            gz = int(2 + tz)
            assert abs(gz) == M.RANGE - 1 and e["k"][0, 2] == gz >> 10 and e["sum"][0, 2] == gz & 1023
    # below min_disp16, a disparity of 0 and the invalid value contribute nothing
    m = np.array([[0, 15, INV, 16]], np.int16)
    e, st = M.fuse([(m, None)], prm, 1.0, 16)
    assert len(e) == 1 and st["n_points"] == 1
    # more voxels than slots: the restatement reports drops
    wide = np.full((1, 1100), 16, np.int16)
    assert M.fuse([(wide, None)], prm, 0.5, 1, capacity_log2=10)[1]["n_dropped"] > 0


def test_additivity_of_the_restatement():
    rng = np.random.default_rng(5)
    prm = _param()
    poses = [None, np.eye(4), POSE, POSE @ POSE, np.linalg.inv(POSE)]
    frames = [(random_map(rng, 9, 31, spread=1500, invalid=0.3), p) for p in poses]
    whole, st = M.fuse(frames, prm, 0.2, 16)
    assert st["n_out_of_range"] == 0
    assert _same(M.fuse(frames[::-1], prm, 0.2, 16)[0], whole)
    for cut in (1, 2, 4):
        a, b = M.fuse(frames[:cut], prm, 0.2, 16)[0], M.fuse(frames[cut:], prm, 0.2, 16)[0]
        assert _same(M.merge(a, b), whole) and _same(M.merge(b, a), whole)
    parts = [M.fuse([fr], prm, 0.2, 16)[0] for fr in frames]
    assert _same(M.merge(*parts), whole) and _same(M.merge(whole), whole)


def test_struct_layouts_and_defaults():
    assert M.ENTRY == MAP_ENTRY_DTYPE and MAP_ENTRY_DTYPE.itemsize == 40
    assert [MAP_ENTRY_DTYPE.fields[n][1] for n in ("k", "count", "sum")] == [0, 12, 16]
    assert [(f[0], getattr(MapParams, f[0]).offset) for f in MapParams._fields_] == [("voxel", 0), ("min_disp16", 8), ("capacity_log2", 12)]
    assert C.sizeof(MapParams) == 16 and C.sizeof(MapCounters) == 40
    assert [f[0] for f in MapCounters._fields_] == ["n_points", "n_inserts", "n_out_of_range", "n_dropped", "n_occupied"]
    L = libviso_amd.load()
    p = MapParams(-1.0, -1, -1)
    L.viso_map_params_default(C.byref(p))
    assert (p.voxel, p.min_disp16, p.capacity_log2) == (0.2, 16, 24) == tuple(MAP_DEFAULTS[k] for k in ("voxel", "min_disp16", "capacity_log2"))
    L.viso_map_params_default(None)
    q = libviso_amd.map_params(voxel=0.05)
    assert (q.voxel, q.min_disp16, q.capacity_log2) == (0.05, 16, 24) and q.ok()
    with pytest.raises(TypeError):
        libviso_amd.map_params(foo=1)


def test_argument_errors_without_a_device():
    L = libviso_amd.load()
    h = C.c_void_p()
    ok = libviso_amd.map_params()
    assert L.viso_map_create(None, None, C.byref(h)) == -1 and L.viso_map_create(None, C.byref(ok), None) == -1
    for bad in (dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(min_disp16=0),
                dict(capacity_log2=9), dict(capacity_log2=29)):
        p = libviso_amd.map_params(**bad)
        assert not p.ok() and L.viso_map_create(None, C.byref(p), C.byref(h)) == -1 and h.value is None, bad
        assert b"viso_map_create" in L.viso_last_error()
    assert L.viso_map_create(C.c_void_p(12345), C.byref(ok), C.byref(h)) == -1     # not a context
    # a handle that is not a map: every call answers, none follows the pointer
    fake = C.c_void_p(4096)
    m = np.zeros((4, 5), np.int16)
    mp = m.ctypes.data_as(C.POINTER(C.c_int16))
    prm = _param()
    n = C.c_size_t()
    e = np.zeros(1, MAP_ENTRY_DTYPE); e["count"] = 1
    st = MapCounters()
    T = np.eye(4)
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    for handle in (None, fake):
        assert L.viso_map_clear(handle) == -1
        assert L.viso_map_fuse(handle, mp, 4, 5, C.byref(prm), None) == -1
        assert L.viso_map_add_entries(handle, e.ctypes.data, 1) == -1
        assert L.viso_map_count(handle, 1, C.byref(n)) == -1
        assert L.viso_map_get(handle, 1, e.ctypes.data, 1, C.byref(n)) == -1
        assert L.viso_map_stats(handle, C.byref(st)) == -1
        assert L.viso_batch_fuse_disparities(None, handle, 0, 1, Tp) == -1
    assert b"viso_batch_fuse_disparities" in L.viso_last_error()
    assert L.viso_map_destroy(None) == 1 and L.viso_map_destroy(fake) == -1
    assert b"viso_map_destroy" in L.viso_last_error()
    # the centroid's own checks
    out = np.zeros(3, np.float32)
    op = out.ctypes.data_as(C.POINTER(C.c_float))
    assert L.viso_map_entry_centroid(None, 0.2, op) == -1 and L.viso_map_entry_centroid(e.ctypes.data, 0.2, None) == -1
    assert L.viso_map_entry_centroid(e.ctypes.data, 0.0, op) == -1 and L.viso_map_entry_centroid(e.ctypes.data, float("nan"), op) == -1
    z = np.zeros(1, MAP_ENTRY_DTYPE)
    assert L.viso_map_entry_centroid(z.ctypes.data, 0.2, op) == -1 and b"viso_map_entry_centroid" in L.viso_last_error()
    assert L.viso_map_entry_centroid(e.ctypes.data, 0.2, op) == 1
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        libviso_amd.VoxelMap(voxel=-1.0)
    with pytest.raises(TypeError):
        libviso_amd.VoxelMap(params=libviso_amd.map_params(), voxel=0.1)


def test_centroid_equals_restatement_bit_for_bit():
    rng = np.random.default_rng(11)
    n = 4000
    e = np.zeros(n, MAP_ENTRY_DTYPE)
    e["k"] = rng.integers(-M.BIAS, M.BIAS, (n, 3))
    e["k"][:4] = [[-M.BIAS] * 3, [M.BIAS - 1] * 3, [0, 0, 0], [-1, -1, -1]]
    e["count"] = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    e["count"][:8] = [1, 1, 1, 3, 7, 2 ** 32 - 1, 2, 5]
    e["sum"] = (rng.random((n, 3)) * 1023 * e["count"][:, None]).astype(np.uint64)
    e["sum"][1] = 1023
    e["sum"][5] = 1023 * (2 ** 32 - 1)
    for voxel in (0.05, 0.2, 1.0, 1000.0, 1e-3):
        got = libviso_amd.map_entry_centroids(e, voxel)
        want = M.centroids(e, voxel)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), voxel
    # the centroid lies inside its voxel (up to the one rounding to float32)
    c = M.centroids(e, 0.2).astype(np.float64)
    lo = e["k"] * 0.2
    assert (c >= lo - 1e-2).all() and (c <= lo + 0.2 + 1e-2).all()


def _png16(values, filters):
    """A 16-bit grayscale PNG of uint16 [rows][cols] whose row y uses filter filters[y % len(filters)]."""
    rows, cols = values.shape
    raw = values.astype(">u2").view(np.uint8).reshape(rows, 2 * cols).astype(np.int32)
    lines = []
    for y in range(rows):
        ft = filters[y % len(filters)]
        cur, up = raw[y], raw[y - 1] if y else np.zeros(2 * cols, np.int32)
        a = np.concatenate([[0, 0], cur[:-2]])
        c = np.concatenate([[0, 0], up[:-2]])
        if ft == 0:
            pred = 0
        elif ft == 1:
            pred = a
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (a + up) >> 1
        else:
            p = a + up - c
            pa, pb, pc = np.abs(p - a), np.abs(p - up), np.abs(p - c)
            pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, up, c))
        lines.append(bytes([ft]) + ((cur - pred) & 255).astype(np.uint8).tobytes())
    chunk = lambda kind, body: struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))   # noqa: E731
    z = zlib.compress(b"".join(lines))
    half = len(z) // 2
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 16, 0, 0, 0, 0)) + chunk(b"tEXt", b"k\0v") +
            chunk(b"IDAT", z[:half]) + chunk(b"IDAT", z[half:]) + chunk(b"IEND", b""))


def test_tool_readers(tmp_path):
    from libviso_amd.kitti_shard import load_host
    import disparity_ref as DR
    H = load_host()
    rng = np.random.default_rng(3)
    for shape in ((1, 1), (7, 13), (200, 400)):
        d = random_map(rng, *shape, spread=16 * 200, invalid=0.3)
        d.flat[0] = 0
        f = str(tmp_path / "d.png")
        assert H.viso_write_disparity_png(f.encode(), d.ctypes.data_as(C.POINTER(C.c_int16)), shape[0], shape[1]) == 1
        got = fuse_map.read_disparity_png(f)
        want = np.where(d <= 0, INV, d).astype(np.int16)     # a disparity of 0 is stored as 0: invalid in the file
        assert got.dtype == np.int16 and np.array_equal(got, want)
        assert np.array_equal(fuse_map.read_png16(f), DR.read_disparity_png(f))
    # all five row filters, two IDAT chunks, an ancillary chunk
    v = rng.integers(0, 65536, (11, 9)).astype(np.uint16)
    for filters in ((0,), (1,), (2,), (3,), (4,), (4, 3, 2, 1, 0)):
        f = tmp_path / "f.png"
        f.write_bytes(_png16(v, filters))
        assert np.array_equal(fuse_map.read_png16(str(f)), v), filters
    for bad in (b"not a png", _png16(v, (0,))[:-20], _png16(v, (0,)).replace(b"\x10\x00\x00\x00\x00", b"\x08\x00\x00\x00\x00", 1)):
        f = tmp_path / "bad.png"
        f.write_bytes(bad)
        with pytest.raises(ValueError):
            fuse_map.read_png16(str(f))
    # the pose file and calib.txt
    p = tmp_path / "poses.txt"
    p.write_text("1 0 0 0.5 0 1 0 -2 0 0 1 3.25\n" + " ".join("%f" % x for x in POSE[:3].reshape(-1)) + "\n")
    T = fuse_map.read_poses(str(p))
    assert T.shape == (2, 4, 4) and T[0, :3, 3].tolist() == [0.5, -2.0, 3.25] and T[1, 3].tolist() == [0, 0, 0, 1]
    assert np.allclose(T[1], POSE, atol=1e-6)
    p.write_text("1 2 3\n")
    with pytest.raises(ValueError):
        fuse_map.read_poses(str(p))
    c = tmp_path / "calib.txt"
    c.write_text("P0: 700 0 600.5 0 0 700 180.25 0 0 0 1 0\nP1: 700 0 600.5 -350 0 700 180.25 0 0 0 1 0\nP2: 1 2 3\n")
    assert fuse_map.read_calib(str(c)) == (700.0, 600.5, 180.25, 0.5)
    c.write_text("P0: 1 2 3\n")
    with pytest.raises(ValueError):
        fuse_map.read_calib(str(c))


def test_ply_header_and_size(tmp_path):
    rng = np.random.default_rng(2)
    e, _ = M.fuse([(random_map(rng, 12, 40, spread=1500, invalid=0.2), POSE)], _param(), 0.2, 16)
    assert len(e) > 10
    data = M.ply_bytes(e, 0.2)
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and f"element vertex {len(e)}" in lines
    assert [ln for ln in lines if ln.startswith("property")] == ["property float x", "property float y", "property float z", "property uint count"]
    assert len(body) == 16 * len(e)
    v = np.frombuffer(body, np.dtype([("xyz", "<f4", (3,)), ("count", "<u4")]))
    assert np.array_equal(v["xyz"], M.centroids(e, 0.2)) and np.array_equal(v["count"], e["count"])
    assert libviso_amd.map_ply_bytes(e, 0.2) == data
    f = tmp_path / "m.ply"
    libviso_amd.write_map_ply(str(f), e, 0.2)
    assert f.read_bytes() == data
    assert M.ply_bytes(e[:0], 0.2).endswith(b"element vertex 0\nproperty float x\nproperty float y\nproperty float z\nproperty uint count\nend_header\n")


def test_kernels_have_no_scratch():
    shared = ("add_entries", "compact", "clear", "evict_mark", "evict_rebuild", "evict_sweep")   # voxel_hash.h's templates, by mangled name
    names = ("map_fuse_kernel",) + tuple(f"voxel_{k}_kernelI10MapPayload" for k in shared)
    res = kernel_resources("voxelmap.hip", names)
    for name, (occ, scratch) in res.items():
        print(f"{name}: occupancy {occ}, scratch {scratch}")
        assert scratch == 0 and occ >= 1


def test_device_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(libviso_amd.VisoError, match="-2"):
        libviso_amd.VoxelMap(voxel=0.2)
