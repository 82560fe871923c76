"""The gray TSDF map without a device (include/viso_hip.h, "TSDF intensity"): the restatement of tests/gray_ref.py against itself
(vectorised against loop), against the plain restatements (tests/tsdf_ref.py, tests/render_ref.py, tests/mesh_ref.py) and against
known answers on walls; the struct layout, the prototypes and the argument checks of the library that need no device; the PLY and
PNG bytes; the resources of the new kernels."""
import ctypes as C
import os

import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map
from libviso_amd.abi import TSDF_ENTRY_DTYPE, TSDF_GRAY_ENTRY_DTYPE, TSDF_MESH_VERTEX_DTYPE, Param

import gray_cases as GC
import gray_ref as G
import mesh_ref as MR
import render_ref as RR
import tsdf_ref as R
from estimator_util import kernel_resources
from test_speckle_cpu import random_map

POSE = GC.POSE
GRAY_KERNELS = ("tsdf_gray_fuse_kernel", "tsdf_gray_sample_kernel", "tsdf_gray_render_kernel")
# the gray map's instances of voxel_hash.h's templates, by mangled name
GRAY_SHARED = tuple(f"voxel_{k}_kernelI11TsdfPayloadILb1EE" for k in ("add_entries", "compact", "clear", "evict_mark", "evict_rebuild", "evict_sweep"))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _image(rng, shape):
    im = rng.integers(0, 256, shape).astype(np.uint8)
    im.flat[0], im.flat[-1] = 0, 255
    return im


def _frames(rng, rows, cols, poses):
    return [(random_map(rng, rows, cols, spread=2100, invalid=0.2), _image(rng, (rows, cols)), pose) for pose in poses]


@pytest.mark.parametrize("seed", range(4))
def test_vectorised_equals_loop_and_plain(seed):
    rng = np.random.default_rng(seed)
    rows, cols = int(rng.integers(1, 9)), int(rng.integers(2, 30))
    frames = _frames(rng, rows, cols, (None, np.eye(4), POSE))
    frames[0][0].flat[0] = 16 * 600          # a point 0.65 m ahead: samples with zj <= 0 at T = 8
    prm = GC.param()
    for voxel, trunc, md in ((0.05, 3, 16), (0.2, 1, 1), (0.2, 3, 16), (0.2, 8, 160), (1000.0, 2, 1)):
        a, sa = G.fuse(frames, prm, voxel, trunc, md)
        b, sb = G.fuse_loop(frames, prm, voxel, trunc, md)
        assert a.dtype == G.ENTRY and _same(a, b) and sa == sb
        # (k, weight, sum) and the statistics are the plain map's, bit for bit
        p, sp = R.fuse([(m, pose) for m, _, pose in frames], prm, voxel, trunc, md)
        assert _same(G.plain(a), p) and sa == sp
        assert (a["gray"] <= 255 * a["weight"].astype(np.uint64)).all() and G.entry_ok(a, trunc).all()
        total = sum(int(im[(m != R.INVALID) & (m >= md)].sum()) for m, im, _ in frames)
        assert voxel < 100 or int(a["gray"].sum()) <= total * (4 * trunc + 1)
        assert _same(G.fuse(frames, prm, voxel, trunc, md, min_weight=2)[0], a[a["weight"] >= 2])


def test_gray_sum_by_hand():
    """One pixel on the optical axis (base 1, d = 1 px, cu = cv = 0, f = 10.25) is a point at Z = 10.25.  At voxel 1 and T = 1 its
    samples enter the voxels kz = 9, 10 and 11, whose centres are 0.75 before, 0.25 behind and 1.25 behind it: q = 768, -256 and,
    beyond the band, no update.  Each voxel is updated once, so its gray sum is the pixel's intensity; a second frame adds its own."""
    prm = Param.default(base=1.0, f=10.25, cu=0.0, cv=0.0)
    m = np.full((3, 4), R.INVALID, np.int16)
    m[0, 0] = 16
    im = np.zeros((3, 4), np.uint8)
    im[0, 0] = 201
    e, _ = G.fuse([(m, im, None)], prm, 1.0, 1, 1)
    assert e["k"].tolist() == [[0, 0, 9], [0, 0, 10]] and e["sum"].tolist() == [768, -256]
    assert (e["weight"] == 1).all() and (e["gray"] == 201).all()
    im2 = im.copy()
    im2[0, 0] = 255
    e2, _ = G.fuse([(m, im, None), (m, im2, None)], prm, 1.0, 1, 1)
    assert (e2["weight"] == 2).all() and (e2["gray"] == 456).all() and _same(e2["sum"], 2 * e["sum"])


def test_additivity_and_order():
    rng = np.random.default_rng(5)
    prm = GC.param()
    frames = _frames(rng, 9, 31, (None, np.eye(4), POSE, POSE @ POSE, np.linalg.inv(POSE)))
    whole, st = G.fuse(frames, prm, 0.2, 3, 16)
    assert st["n_out_of_range"] == 0 and len(whole) > 100
    assert _same(G.fuse(frames[::-1], prm, 0.2, 3, 16)[0], whole)
    for cut in (1, 2, 4):
        a, b = G.fuse(frames[:cut], prm, 0.2, 3, 16)[0], G.fuse(frames[cut:], prm, 0.2, 3, 16)[0]
        assert _same(G.merge(a, b), whole) and _same(G.merge(b, a), whole)
    parts = [G.fuse([fr], prm, 0.2, 3, 16)[0] for fr in frames]
    assert _same(G.merge(*parts), whole) and _same(G.merge(*parts[::-1]), whole) and _same(G.merge(whole), whole)
    assert _same(G.plain(G.merge(*parts)), R.merge(*[G.plain(p) for p in parts]))


def test_edge_gray_rule():
    """The rule's ends and its rounding, by hand and vectorised against one edge at a time."""
    one = lambda *a: int(G.edge_gray(*[np.array([v]) for v in a])[0])
    # t = 0 (sum_a = 0): a's mean; equal distances: the middle, halves rounded up; 255 stays 255
    assert one(2, 0, 2 * 100, 1, -5, 30) == 100 and G.edge_gray_1(2, 0, 200, 1, -5, 30) == 100
    assert one(1, 512, 10, 1, -512, 11) == 11                # 10.5 -> 11
    assert one(1, 512, 255, 1, -512, 255) == 255 and one(3, -7, 0, 2, 9, 0) == 0
    assert one(1, -512, 0, 1, 512, 255) == 128               # a negative, b positive: 127.5 -> 128
    rng = np.random.default_rng(3)
    n = 2000
    wa, wb = rng.integers(1, 50, n), rng.integers(1, 50, n)
    sa, sb = rng.integers(0, 3072, n) * wa, -rng.integers(1, 3072, n) * wb
    flip = rng.random(n) < 0.5
    sa, sb = np.where(flip, -sa - 1, sa), np.where(flip, -sb - 1, sb)
    ga, gb = rng.integers(0, 256, n) * wa - rng.integers(0, 2, n) * (wa > 1), rng.integers(0, 256, n) * wb
    ga = np.maximum(ga, 0)
    v = G.edge_gray(wa, sa, ga, wb, sb, gb)
    assert v.dtype == np.uint8 and [int(x) for x in v] == [G.edge_gray_1(*t) for t in zip(wa, sa, ga, wb, sb, gb)]
    lo, hi = np.minimum(ga / wa, gb / wb), np.maximum(ga / wa, gb / wb)
    assert (v >= np.floor(lo)).all() and (v <= np.ceil(hi)).all()


def test_vertex_gray_of_the_restatement():
    rng = np.random.default_rng(8)
    prm = GC.param()
    e, _ = G.fuse(_frames(rng, 12, 40, (POSE,)), prm, 0.2, 3, 16)
    v, tri = MR.mesh(G.plain(e), 0.2)
    c = R.crossings(G.plain(e))
    assert len(v) > 10 and len(c) > 10
    g, missing = G.vertex_gray(e, v)
    assert missing == 0 and g.dtype == np.uint8
    table = {tuple(x["k"].tolist()): (int(x["weight"]), int(x["sum"]), int(x["gray"])) for x in e}
    for i in range(len(v)):
        d = int(v["dir"][i])
        a = tuple(v["k"][i].tolist())
        b = (a[0] + (d & 1), a[1] + (d >> 1 & 1), a[2] + (d >> 2))
        assert int(g[i]) == G.edge_gray_1(*table[a], *table[b])
    gc, missing = G.vertex_gray(e, G.crossing_vertices(c))
    assert missing == 0
    assert [int(x) for x in gc] == [G.edge_gray_1(int(x["wa"]), int(x["sa"]), table[tuple(x["k"].tolist())][2], int(x["wb"]), int(x["sb"]),
                                                  table[tuple((x["k"] + np.eye(3, dtype=np.int32)[x["axis"]]).tolist())][2]) for x in c]
    # an absent end and ends of one sign are missing, with 0
    odd = np.zeros(3, G.VERTEX)
    odd["k"], odd["dir"] = [e["k"][0], e["k"][0] - 50, v["k"][0]], [7, 1, v["dir"][0]]
    same = np.nonzero((np.diff(G.keys_of(e["k"])) == 1) & ((e["sum"][:-1] < 0) == (e["sum"][1:] < 0)))[0]
    odd["k"][0], odd["dir"][0] = e["k"][same[0]], 4            # the neighbour along z has the same sign
    g3, missing = G.vertex_gray(e, odd)
    assert missing == 2 and g3[0] == 0 and g3[1] == 0 and g3[2] == g[0]
    bad = np.zeros(6, G.VERTEX)
    bad["dir"] = [0, 8, 1, 2, 4, 1]
    bad["k"][2:5] = [[R.BIAS - 1, 0, 0], [0, R.BIAS - 1, 0], [0, 0, R.BIAS - 1]]
    bad["k"][5] = [-R.BIAS - 1, 0, 0]
    assert not G.vertex_ok(bad).any()
    fine = np.zeros(3, G.VERTEX)
    fine["dir"], fine["k"] = [6, 1, 7], [[R.BIAS - 1, 0, 0], [R.BIAS - 2, R.BIAS - 1, R.BIAS - 1], [-R.BIAS] * 3]
    assert G.vertex_ok(fine).all()


@pytest.mark.parametrize("seed", range(2))
def test_render_vectorised_equals_loop_and_plain(seed):
    rng = np.random.default_rng(20 + seed)
    prm = Param.default(base=0.5371, f=60.0, cu=14.5, cv=5.5)
    m = np.full((12, 30), 16 * 12, np.int16)                   # a wall 2.7 m ahead, with holes
    m[rng.random(m.shape) < 0.1] = R.INVALID
    m[:, 20:] = 16 * 20
    im = _image(rng, m.shape)
    e, _ = G.fuse([(m, im, POSE if seed else None)], prm, 0.2, 3, 16)
    for pose, mw in ((POSE if seed else None, 1), (RR.sideways(POSE if seed else None, 0.1, 0.03), 1), (None, 2)):
        d, w, g = G.render(e, 0.2, prm, m.shape, pose, 5.0, mw)
        d2, w2, g2 = G.render_loop(e, 0.2, prm, m.shape, pose, 5.0, mw)
        assert _same(d, d2) and _same(w, w2) and _same(g, g2) and g.dtype == np.uint8
        dp, wp = RR.render(G.plain(e), 0.2, prm, m.shape, pose, 5.0, mw)
        assert _same(d, dp) and _same(w, wp)
        assert (g[d == R.INVALID] == 0).all()
        assert pose is not None and seed == 0 or mw > 1 or (d != R.INVALID).sum() > 50


@pytest.mark.parametrize("name,pose", GC.CASES)
def test_known_answers_on_walls(name, pose):
    m, voxel, max_depth, Z = GC.wall(name)
    T, prm, w = GC.POSES[pose], GC.param(), GC.window(name)
    plain_e = None
    for tag, im in GC.images().items():
        e, st = G.fuse([(m, im, T)], prm, voxel, GC.TRUNC, 16)
        assert st["n_out_of_range"] == 0 and st["n_points"] == m.size
        if plain_e is None:
            plain_e = R.fuse([(m, T)], prm, voxel, GC.TRUNC, 16)[0]
            want_d, want_w = RR.render(plain_e, voxel, prm, GC.SHAPE, T, max_depth, 1)
        assert _same(G.plain(e), plain_e)
        d, wt, g = G.render(e, voxel, prm, GC.SHAPE, T, max_depth, 1)
        assert _same(d, want_d) and _same(wt, want_w)
        worst = GC.check_render(f"{name}/{pose}/{tag}", im, w, d, g)
        v, _ = MR.mesh(plain_e, voxel)
        gv, missing = G.vertex_gray(e, v)
        assert missing == 0 and len(v) > 0
        if tag == "const":
            c = int(im.flat[0])
            assert (e["gray"] == np.uint64(c) * e["weight"].astype(np.uint64)).all()
            assert (gv == c).all() and (g[d != R.INVALID] == c).all() and worst == 0
        else:
            assert int(gv.min()) >= int(im.min()) and int(gv.max()) <= int(im.max())


def test_struct_layout_and_prototypes():
    assert G.ENTRY == TSDF_GRAY_ENTRY_DTYPE and TSDF_GRAY_ENTRY_DTYPE.itemsize == 32
    assert [TSDF_GRAY_ENTRY_DTYPE.fields[n][1] for n in ("k", "weight", "sum", "gray")] == [0, 12, 16, 24]
    assert G.PLAIN == TSDF_ENTRY_DTYPE and G.VERTEX == TSDF_MESH_VERTEX_DTYPE
    L = libviso_amd.load()
    want = {"viso_tsdf_create_gray": 3, "viso_tsdf_is_gray": 2, "viso_tsdf_fuse_gray": 7, "viso_tsdf_get_gray": 5,
            "viso_tsdf_add_gray_entries": 3, "viso_tsdf_vertex_gray": 5, "viso_tsdf_render_gray": 11}
    for name, n_args in want.items():
        assert len(getattr(L, name).argtypes) == n_args, name
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "viso_hip.h")).read()
    for name in want:
        assert f"int {name}(" in header, name
    section = header[header.index("TSDF intensity: "):]
    for name in GRAY_KERNELS:
        assert name in section, name
    assert "colour" not in header.replace('"colour" is one intensity', "")


def test_argument_errors_without_a_device():
    L = libviso_amd.load()
    h = C.c_void_p()
    ok = libviso_amd.tsdf_params()
    assert L.viso_tsdf_create_gray(None, None, C.byref(h)) == -1 and L.viso_tsdf_create_gray(None, C.byref(ok), None) == -1
    for bad in (dict(voxel=0.0), dict(voxel=float("nan")), dict(trunc_voxels=0), dict(trunc_voxels=9), dict(min_disp16=0),
                dict(capacity_log2=9), dict(capacity_log2=29)):
        p = libviso_amd.tsdf_params(**bad)
        assert L.viso_tsdf_create_gray(None, C.byref(p), C.byref(h)) == -1 and h.value is None, bad
        assert b"viso_tsdf_create_gray" in L.viso_last_error()
    assert L.viso_tsdf_create_gray(C.c_void_p(12345), C.byref(ok), C.byref(h)) == -1     # not a context
    # a handle that is not a TSDF map: every new call answers, none follows the pointer
    fake = C.c_void_p(4096)
    m, im = np.zeros((4, 5), np.int16), np.zeros((4, 5), np.uint8)
    mp, ip = m.ctypes.data_as(C.POINTER(C.c_int16)), im.ctypes.data_as(C.POINTER(C.c_uint8))
    prm = GC.param()
    n, kind = C.c_size_t(), C.c_int(7)
    e = np.zeros(1, TSDF_GRAY_ENTRY_DTYPE); e["weight"] = 1
    v = np.zeros(1, TSDF_MESH_VERTEX_DTYPE); v["dir"] = 1
    g = np.zeros(20, np.uint8)
    gp = g.ctypes.data_as(C.POINTER(C.c_uint8))
    for handle in (None, fake):
        assert L.viso_tsdf_is_gray(handle, C.byref(kind)) == -1 and kind.value == 7
        assert L.viso_tsdf_fuse_gray(handle, mp, ip, 4, 5, C.byref(prm), None) == -1
        assert L.viso_tsdf_add_gray_entries(handle, e.ctypes.data, 1) == -1
        assert L.viso_tsdf_get_gray(handle, 1, e.ctypes.data, 1, C.byref(n)) == -1
        assert L.viso_tsdf_vertex_gray(handle, v.ctypes.data, 1, gp, C.byref(n)) == -1
        assert L.viso_tsdf_render_gray(handle, 1, C.byref(prm), 4, 5, 10.0, None, 1, mp, None, gp) == -1
        assert b"viso_tsdf_render_gray" in L.viso_last_error()
    # the render's own checks come before the handle, as viso_tsdf_render's do
    assert L.viso_tsdf_render_gray(fake, 1, C.byref(prm), 4, 5, 10.0, None, 1, mp, None, None) == -1
    assert L.viso_tsdf_render_gray(fake, 0, C.byref(prm), 4, 5, 10.0, None, 1, mp, None, gp) == -1
    assert L.viso_tsdf_render_gray(fake, 1, C.byref(prm), 4, 5, float("nan"), None, 1, mp, None, gp) == -1
    # the wrapper's own checks need no map either
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        libviso_amd.TsdfMap(gray=True, voxel=-1.0)
    with pytest.raises(ValueError):
        libviso_amd.mesh_ply_bytes(np.zeros(2, TSDF_MESH_VERTEX_DTYPE), np.zeros((0, 3), np.uint32), gray=np.zeros(3, np.uint8))
    with pytest.raises(ValueError):
        libviso_amd.mesh_ply_bytes(np.zeros(2, TSDF_MESH_VERTEX_DTYPE), np.zeros((0, 3), np.uint32), gray=np.zeros(2, np.int32))


def test_device_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(libviso_amd.VisoError, match="-2"):
        libviso_amd.TsdfMap(gray=True, voxel=0.2, capacity_log2=10)


def test_ply_header_and_bytes(tmp_path):
    rng = np.random.default_rng(2)
    e, _ = G.fuse(_frames(rng, 12, 40, (POSE,)), GC.param(), 0.2, 3, 16)
    v, tri = MR.mesh(G.plain(e), 0.2)
    c = R.crossings(G.plain(e))
    gv, gc = G.vertex_gray(e, v)[0], G.vertex_gray(e, G.crossing_vertices(c))[0]
    assert len(tri) > 10 and len(c) > 10 and len(set(gv.tolist())) > 5
    rgb = ["property uchar red", "property uchar green", "property uchar blue"]
    xyzw = ["property float x", "property float y", "property float z", "property uint weight"]
    # the mesh
    data = G.mesh_ply_bytes(v, tri, gv)
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and f"element vertex {len(v)}" in lines and f"element face {len(tri)}" in lines
    assert [ln for ln in lines if ln.startswith("property")] == xyzw + rgb + ["property list uchar int vertex_indices"]
    assert lines.index("property uchar blue") < lines.index(f"element face {len(tri)}")
    assert len(body) == 19 * len(v) + 13 * len(tri)
    rec = np.frombuffer(body[:19 * len(v)], np.dtype([("xyz", "<f4", (3,)), ("weight", "<u4"), ("rgb", "u1", (3,))]))
    assert np.array_equal(rec["xyz"], v["p"]) and np.array_equal(rec["weight"], v["weight"]) and (rec["rgb"] == gv[:, None]).all()
    assert libviso_amd.mesh_ply_bytes(v, tri, gv) == data and libviso_amd.mesh_ply_bytes(v, tri, gray=gv) == data
    f = tmp_path / "m.ply"
    libviso_amd.write_mesh_ply(str(f), v, tri, gv)
    assert f.read_bytes() == data
    # the surface
    data = G.surface_ply_bytes(c, 0.2, gc)
    head, _, body = data.partition(b"end_header\n")
    assert [ln for ln in head.decode("ascii").split("\n") if ln.startswith("property")] == xyzw + rgb and len(body) == 19 * len(c)
    assert libviso_amd.surface_ply_bytes(c, 0.2, gc) == data
    libviso_amd.write_surface_ply(str(f), c, 0.2, gray=gc)
    assert f.read_bytes() == data
    # without the intensity the bytes are the plain files'
    assert libviso_amd.mesh_ply_bytes(v, tri) == MR.ply_bytes(v, tri) == libviso_amd.mesh_ply_bytes(v, tri, None)
    assert libviso_amd.surface_ply_bytes(c, 0.2) == R.ply_bytes(c, 0.2) == libviso_amd.surface_ply_bytes(c, 0.2, None)
    libviso_amd.write_mesh_ply(str(f), v, tri)
    assert f.read_bytes() == MR.ply_bytes(v, tri)
    assert G.mesh_ply_bytes(v[:0], tri[:0], gv[:0]) == libviso_amd.mesh_ply_bytes(v[:0], tri[:0], gv[:0])


def _png8_with_filters(path, v, filters):
    """An 8-bit grayscale PNG of v whose row y is filtered with filters[y % len(filters)] (the PNG specification's five; any other
    number is written as the row's filter byte before the plain row)."""
    import struct
    import zlib
    rows, cols = v.shape
    raw = bytearray()
    for y in range(rows):
        ft = filters[y % len(filters)]
        line = [int(x) for x in v[y]]
        up = [int(x) for x in v[y - 1]] if y else [0] * cols
        out = []
        for i in range(cols):
            a, b, c = (line[i - 1] if i else 0), up[i], (up[i - 1] if i else 0)
            p = a + b - c
            paeth = a if abs(p - a) <= abs(p - b) and abs(p - a) <= abs(p - c) else b if abs(p - b) <= abs(p - c) else c
            out.append((line[i] - (0, a, b, (a + b) >> 1, paeth)[ft if ft < 5 else 0]) & 255)
        raw += bytes([ft] + out)
    chunk = lambda kind, body: struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 8, 0, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(bytes(raw))) + chunk(b"IEND", b""))


def test_png8_round_trip_and_filters(tmp_path):
    rng = np.random.default_rng(4)
    p = str(tmp_path / "a.png")
    for shape in ((1, 1), (7, 13), (40, 130)):
        v = _image(rng, shape)
        fuse_map.write_png8(p, v)
        got = fuse_map.read_png8(p)
        assert got.dtype == np.uint8 and np.array_equal(got, v)
        for filters in ((0,), (1,), (2,), (3,), (4,), (4, 3, 2, 1, 0)):
            _png8_with_filters(p, v, filters)
            assert np.array_equal(fuse_map.read_png8(p), v), (shape, filters)
    # anything else is refused: a 16-bit file by the 8-bit reader and the other way round, a wrong array by the writer
    fuse_map.write_png16(p, np.arange(12, dtype=np.uint16).reshape(3, 4))
    with pytest.raises(ValueError, match="8-bit"):
        fuse_map.read_png8(p)
    fuse_map.write_png8(p, np.zeros((3, 4), np.uint8))
    with pytest.raises(ValueError, match="16-bit"):
        fuse_map.read_png16(p)
    _png8_with_filters(p, np.zeros((3, 4), np.uint8), (5,))
    with pytest.raises(ValueError, match="row filter"):
        fuse_map.read_png8(p)
    for bad in (np.zeros((3, 4), np.uint16), np.zeros(4, np.uint8), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            fuse_map.write_png8(p, bad)
    with open(p, "wb") as f:
        f.write(b"not a png")
    with pytest.raises(ValueError):
        fuse_map.read_png8(p)


def test_new_kernels_have_no_scratch():
    res = kernel_resources("tsdf.hip", GRAY_KERNELS + GRAY_SHARED)
    for name, (occ, scratch) in res.items():
        print(f"{name}: occupancy {occ}, scratch {scratch}")
        assert scratch == 0 and occ >= 1
