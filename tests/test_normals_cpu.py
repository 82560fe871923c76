"""The surface normals of the TSDF map (include/viso_hip.h, "TSDF normals") without a device: the two numpy restatements
(tests/normal_ref.py) against each other, the branches of the rule they meet on the hand-built tables, the accuracy of the method
against the analytic normal of planes, the refusals of the C ABI that touch no device, the PLY writers and shade_normals."""
import ctypes as C
import hashlib
from collections import Counter

import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map, hostmath
from libviso_amd.abi import TSDF_MESH_VERTEX_DTYPE, Param

import mesh_ref as MR
import normal_ref as N
import render_ref as RR
import tsdf_ref as R
import tsdf_tables as TT

INV = R.INVALID
POSE = np.linalg.inv(hostmath.tr2mat([0.013, -0.021, 0.007, 0.31, -0.12, 1.47]))   # the pose of test_gpu_tsdf
SHAPE = (37, 333)


def _param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the two forms agree -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 130), (1, 1)])
def test_the_two_restatements_agree_on_renders(shape):
    """The views are windows of the fused 37 x 333 maps (normal_ref.window): a map fused from three rows is one voxel thick, and
    no voxel of it has a gradient."""
    prm = _param()
    win = N.window(prm, shape, SHAPE, 0.1)
    n_normals = 0
    for i, name in enumerate(RR.SCENES):
        fuse_pose = (None, POSE)[i % 2]
        frames = [(RR.scene_map(name, SHAPE, 0.1), fuse_pose)]
        frames.append((frames[0][0], RR.sideways(fuse_pose, 0.02)))
        e, st = R.fuse(frames, prm, 0.2, 3, 16)
        assert st["n_out_of_range"] == 0
        for view in (fuse_pose, RR.sideways(fuse_pose, 0.1, 0.01)):
            for mw in (1, 2):
                a = N.render(e, 0.2, win, shape, view, 17.0, mw)
                b = N.render_loop(e, 0.2, win, shape, view, 17.0, mw)
                assert a[2].dtype == np.float32 and a[2].shape == shape + (3,)
                assert all(_same(x, y) for x, y in zip(a, b)), (name, mw)
                assert not a[2][a[0] == INV].any()
                n_normals += int(a[2].any(axis=-1).sum())
    assert n_normals >= (8 if shape == (1, 1) else 2000), n_normals


def test_the_two_restatements_agree_on_a_mesh():
    e = MR.sphere_entries()
    v, _ = MR.mesh(e, 0.2)
    c = N.crossing_vertices(R.crossings(e))
    for vertices in (v, c):
        a, ma = N.vertex_normals(e, vertices)
        b, mb = N.vertex_normals_loop(e, vertices)
        assert _same(a, b) and ma == mb and len(a) > 200 and ma < len(a) // 2
    # a sphere's normals point away from its centre (the distance is positive outside)
    n, _ = N.vertex_normals(e, v)
    has = n.any(axis=-1)
    out = v["p"][has].astype(np.float64) - 5.3 * 0.2 - 0.1
    assert ((n[has] * out).sum(axis=1) > 0).all()


# ---- branch coverage ---------------------------------------------------------------------------------------------------------------
def every_edge(entries, rng, n=600):
    """A list of (k, dir) around the voxels of a table, most of whose ends are absent or of one sign."""
    e = entries[rng.integers(0, len(entries), n)]
    v = np.zeros(n, MR.VERTEX)
    v["k"], v["dir"] = e["k"] - rng.integers(0, 2, (n, 3)), rng.integers(1, 8, n)
    return v[N.vertex_ok(v)]


def branch_trace():
    """(Counter of normal_ref.BRANCHES, [(tag, entries, vertices, min_weight)]) over the hand-built tables: the random blocks at the
    origin and at both ends of the key range at min_weight 1, 2, 3 with their mesh vertices, their crossings and edges whose ends
    are absent, and normal_ref.flat_table for the normal of length zero, which no random block meets.  Shared with the device test."""
    trace, cases = Counter(), []
    for place in TT.CROSSING_PLACES:
        e = TT.crossing_block(place)
        for mw in TT.BLOCK_MIN_WEIGHTS:
            lists = (MR.mesh(e, 0.2, mw)[0], N.crossing_vertices(R.crossings(e, mw)), every_edge(e, np.random.default_rng(mw)))
            for j, v in enumerate(lists):
                cases.append(((place, mw, j), e, v, mw))
    cases.append((("flat",),) + N.flat_table() + (1,))
    for tag, e, v, mw in cases:
        a, ma = N.vertex_normals(e, v, mw)
        b, mb = N.vertex_normals_loop(e, v, mw, trace)
        assert _same(a, b) and ma == mb, tag
    return trace, cases


def test_hand_built_tables_reach_every_branch():
    trace, _ = branch_trace()
    assert set(trace) == set(N.BRANCHES) and all(trace[b] > 0 for b in N.BRANCHES), dict(trace)
    # the ray casting over the random blocks meets the gradient's branches too
    rays = Counter()
    for _, mw, case in TT.block_sweep("inside"):
        a, b = N.render(*case), N.render_loop(*case, trace=rays)
        assert all(_same(x, y) for x, y in zip(a, b))
    assert all(rays[b] > 0 for b in ("central", "up_only", "down_only", "no_gradient", "normal")), dict(rays)
    # the table of the missing length: the first edge has none, the second has one
    e, v = N.flat_table()
    n, missing = N.vertex_normals(e, v)
    assert missing == 1 and not n[0].any() and n[1].any()


def test_min_weight_decides_what_is_usable():
    e = TT.crossing_block("origin")
    v = MR.mesh(e, 0.2, 1)[0]
    n1, m1 = N.vertex_normals(e, v, 1)
    n2, m2 = N.vertex_normals(e, v, 2)
    assert m2 > m1 and not _same(n1, n2)
    assert _same(n2, N.vertex_normals(e[e["weight"] >= 2], v, 1)[0])


# ---- the accuracy of the method ----------------------------------------------------------------------------------------------------
def _plane_normal(name):
    """The unit normal of a scene of one piece in the world frame, towards the camera at POSE that measured it: in that camera's
    coordinates the plane is n . P = f base with n = (g f, 0, p - g xm + g cu) (render_ref.ideal), and the camera is on its side
    n . P < f base."""
    prm = _param()
    (p, g, _, _), = RR._parts(name, SHAPE[1])
    n = np.array([g * prm.f, 0.0, p - g * (SHAPE[1] - 1) / 2.0 + g * prm.cu])
    return POSE[:3, :3] @ (-n / np.linalg.norm(n))


def _angles(n, truth):
    n = n.astype(np.float64)
    return np.degrees(np.arccos(np.clip((n * truth).sum(axis=-1) / np.linalg.norm(n, axis=-1), -1.0, 1.0)))


# Measured on the restatement (vectorised, voxel 0.2, T = 3, fused from POSE at 37 x 333, max_depth 20, min_weight 1): the largest
# and the median angle in degrees between the normal and the analytic normal of the plane, over the pixels (the vertices) that have a
# normal.  They describe the method (projective distances on a grid of 0.2 m, a gradient over two voxels), not an error of the code;
# DESIGN.md 5.23 has them.  The wall is fronto-parallel to the fusing camera, so its projective distance is the true one up to
# the floor of the fuse's step 6; the plane is slanted by 0.03 px a column, 22 degrees against the fusing camera's axis.
MEASURED = {("wall", "same"): (0.0474, 0.0108), ("wall", "moved"): (0.0474, 0.0108), ("wall", "vertices"): (0.0381, 0.0108),
            ("plane", "same"): (6.443, 0.821), ("plane", "moved"): (6.443, 0.757), ("plane", "vertices"): (7.072, 0.966)}


@pytest.mark.parametrize("name", ["wall", "plane"])
def test_plane_normals_against_the_analytic_normal(name):
    prm = _param()
    e, st = R.fuse([(RR.scene_map(name, SHAPE), POSE)], prm, 0.2, 3, 16)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0
    truth = _plane_normal(name)
    for tag, view in (("same", POSE), ("moved", RR.sideways(POSE, 0.5))):
        d, _, n = N.render(e, 0.2, prm, SHAPE, view, 20.0, 1)
        valid, has = d != INV, n.any(axis=-1)
        assert not (has & ~valid).any()
        a = _angles(n[has], view[:3, :3].T @ truth)
        print(f"{name}, {tag}: {valid.mean():.3f} valid, {has.sum() / valid.sum():.4f} of them with a normal, max {a.max():.4f}, median {np.median(a):.4f} degrees")
        assert has.sum() >= 0.5 * valid.sum() and valid.mean() > 0.5
        assert (n[has][:, 2] < 0).all()                                        # every normal faces the camera
        assert (np.abs(np.linalg.norm(n[has].astype(np.float64), axis=-1) - 1.0) <= 2.0 ** -23).all()
        assert a.max() <= MEASURED[name, tag][0] * 1.25 and np.median(a) <= MEASURED[name, tag][1] * 1.25
    v, _ = MR.mesh(e, 0.2, 1)
    n, missing = N.vertex_normals(e, v, 1)
    has = n.any(axis=-1)
    a = _angles(n[has], truth)
    print(f"{name}, vertices: {len(v)}, {missing} without a normal, max {a.max():.4f}, median {np.median(a):.4f} degrees")
    assert missing == int((~has).sum()) and has.sum() >= 0.5 * len(v) > 0
    assert ((n[has] * (POSE[:3, 3] - v["p"][has].astype(np.float64))).sum(axis=1) > 0).all()   # towards the camera that saw the surface
    assert (np.abs(np.linalg.norm(n[has].astype(np.float64), axis=-1) - 1.0) <= 2.0 ** -23).all()
    assert a.max() <= MEASURED[name, "vertices"][0] * 1.25 and np.median(a) <= MEASURED[name, "vertices"][1] * 1.25


def test_a_pose_rotates_the_world_normals():
    """A render with a pose is the world normals of the same hits, rotated by that pose in the restatement's own doubles; the
    rotation is one of the camera: the hits, not the normals' world directions, depend on it."""
    prm = _param()
    e, _ = R.fuse([(RR.scene_map("plane", SHAPE), POSE)], prm, 0.2, 3, 16)
    view = RR.sideways(POSE, 0.1, 0.01)
    d, w, world, has = N.render_world(e, 0.2, prm, SHAPE, view, 20.0, 1)
    got = N.render(e, 0.2, prm, SHAPE, view, 20.0, 1)
    assert _same(got[0], d) and _same(got[1], w) and has.sum() > 1000
    R3 = view[:3, :3]
    want = np.stack([(R3[0, j] * world[..., 0] + R3[1, j] * world[..., 1]) + R3[2, j] * world[..., 2] for j in range(3)], axis=-1)
    assert _same(got[2], want.astype(np.float32))
    back = got[2][has].astype(np.float64) @ R3.T                                 # and back in the world, up to the float cast
    assert np.abs(back - world[has]).max() < 1e-6
    # the same pose as a translation only: the normals come out as they are in the world
    shift = np.eye(4)
    shift[:3, 3] = view[:3, 3]
    d2, _, world2, has2 = N.render_world(e, 0.2, prm, SHAPE, shift, 20.0, 1)
    assert _same(N.render(e, 0.2, prm, SHAPE, shift, 20.0, 1)[2], np.where(has2[..., None], world2, 0.0).astype(np.float32))


# ---- the C ABI without a device ----------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    L = libviso_amd.load()
    assert len(L.viso_tsdf_vertex_normals.argtypes) == 6 and len(L.viso_tsdf_render_normals.argtypes) == 11
    assert L.viso_tsdf_render_normals.argtypes[5] is C.c_double
    assert isinstance(libviso_amd.TsdfMap.normals, property)
    for name in ("vertices", "surface", "mesh", "render"):
        assert callable(getattr(libviso_amd.TsdfNormals, name))
    for name in ("mesh_normals_ply_bytes", "write_mesh_normals_ply", "surface_normals_ply_bytes", "write_surface_normals_ply"):
        assert callable(getattr(libviso_amd, name))
    assert callable(libviso_amd.shade_normals)


def test_argument_errors_without_a_device():
    """Every argument error of both calls answers VISO_ERR_ARG whatever the handle is, follows no pointer of it and writes nothing."""
    L = libviso_amd.load()
    prm = _param()
    d, w, nrm = np.full((2, 2, 3), 77, np.int16), np.full((2, 2, 3), 77, np.uint32), np.full((2, 2, 3, 3), 77, np.float32)
    T = np.stack([np.eye(4), POSE])
    dp, wp, Tp = d.ctypes.data_as(C.POINTER(C.c_int16)), w.ctypes.data_as(C.POINTER(C.c_uint32)), T.ctypes.data_as(C.POINTER(C.c_double))
    np_ = nrm.ctypes.data_as(C.POINTER(C.c_float))

    def render(handle, min_weight=1, param=prm, rows=2, cols=3, max_depth=10.0, poses=Tp, n_views=2, out=dp, normals=np_):
        return L.viso_tsdf_render_normals(handle, min_weight, C.byref(param) if param is not None else None, rows, cols, max_depth, poses,
                                          n_views, out, wp, normals)

    def bad_param(**kw):
        p = _param()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    Tbad = T.copy()
    Tbad[1, 2, 3] = np.inf
    wrong = [dict(normals=None), dict(out=None), dict(min_weight=0), dict(param=None), dict(rows=0), dict(cols=0), dict(rows=-1),
             dict(rows=65536, cols=65536), dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=np.inf), dict(max_depth=np.nan),
             dict(n_views=0), dict(poses=None, n_views=2), dict(poses=Tbad.ctypes.data_as(C.POINTER(C.c_double))),
             dict(param=bad_param(f=0.0)), dict(param=bad_param(base=0.0)), dict(param=bad_param(cu=np.inf))]
    v = np.zeros(3, TSDF_MESH_VERTEX_DTYPE)
    v["dir"] = 1, 7, 4
    out = np.full((3, 3), 77, np.float32)
    op = out.ctypes.data_as(C.POINTER(C.c_float))
    missing = C.c_size_t(77)

    def vertex(handle, min_weight=1, vertices=v, n=None, normals=op):
        return L.viso_tsdf_vertex_normals(handle, min_weight, vertices.ctypes.data if vertices is not None else None,
                                          len(v) if n is None else n, normals, C.byref(missing))

    def changed(**kw):
        x = v.copy()
        for name, value in kw.items():
            x[name][1] = value
        return x

    top, low = TT.BIAS - 1, -TT.BIAS
    wrong_v = [dict(min_weight=0), dict(normals=None), dict(vertices=None), dict(vertices=changed(dir=0)), dict(vertices=changed(dir=8)),
               dict(vertices=changed(dir=-1)), dict(vertices=changed(k=(0, top + 1, 0))), dict(vertices=changed(k=(low - 1, 0, 0))),
               dict(vertices=changed(k=(0, 0, top))), dict(vertices=changed(k=(top, 0, 0), dir=1)), dict(vertices=changed(k=(0, top, 0), dir=6))]
    for handle in (None, C.c_void_p(4096)):
        for kw in wrong:
            assert render(handle, **kw) == -1, kw
            msg = L.viso_last_error()
            assert b"viso_tsdf_render_normals" in msg and b"bad argument" in msg, (kw, msg)
        assert render(handle) == -1 and b"viso_tsdf_render_normals: not a live TSDF handle" in L.viso_last_error()
        assert render(handle, max_depth=1e9) == -1                              # N beyond 65536 for any voxel a map can have
        for kw in wrong_v:
            assert vertex(handle, **kw) == -1, kw
            msg = L.viso_last_error()
            assert b"viso_tsdf_vertex_normals" in msg and (b"bad argument" in msg or b"is not an edge" in msg), (kw, msg)
        # the last index without the bit set is an edge of the map; a good list meets the handle
        assert vertex(handle, vertices=changed(k=(top, top, 0), dir=4)) == -1 and b"not a live TSDF handle" in L.viso_last_error()
        assert vertex(handle, vertices=changed(k=(low, low, low))) == -1 and b"not a live TSDF handle" in L.viso_last_error()
        assert vertex(handle, n=0, vertices=None, normals=None) == -1 and b"not a live TSDF handle" in L.viso_last_error()
    assert (d == 77).all() and (w == 77).all() and (nrm == 77).all() and (out == 77).all() and missing.value == 77
    # the Python methods raise with the code
    m = object.__new__(libviso_amd.TsdfMap)
    m.L, m.h = L, 4096
    try:
        for call in (lambda: m.normals.render(prm, (2, 3)), lambda: m.normals.vertices(v), lambda: m.normals.vertices(v, min_weight=0)):
            with pytest.raises(libviso_amd.VisoError, match="-1"):
                call()
    finally:
        m.h = None


# ---- the PLY writers ---------------------------------------------------------------------------------------------------------------
# sha256 of what the writers gave for the inputs of _ply_inputs before they took normals: without normals the bytes are those
PLY_BEFORE = {"mesh": "657c2cdc7d70c11a7a3b5d273558fcceaa4198f94f1cf1c15c8a28e851af1cf9",
              "mesh_gray": "0bc975774ba63cdca814a7a8b3772c34340174a9c19b844c5acd859009bfad39",
              "surface": "d81071f0ec26c1cf1a7dc3c3a8e88f3f797b9e89e3e5828b23881632625921df",
              "surface_gray": "39f0d7d6b6bfbe08d120513c2182e2a84c53036a78af4f9c8c8a251ddb40a40c"}


def _ply_inputs():
    e = MR.sphere_entries()
    v, tri = MR.mesh(e, 0.2)
    c = R.crossings(e)
    assert (len(v), len(tri), len(c)) == (758, 1512, 246)
    return e, v, tri, c, (np.arange(len(v)) % 256).astype(np.uint8), (np.arange(len(c)) * 7 % 256).astype(np.uint8)


def test_ply_bytes_without_normals_are_unchanged():
    _, v, tri, c, gv, gc = _ply_inputs()
    got = {"mesh": libviso_amd.mesh_ply_bytes(v, tri), "mesh_gray": libviso_amd.mesh_ply_bytes(v, tri, gv),
           "surface": libviso_amd.surface_ply_bytes(c, 0.2), "surface_gray": libviso_amd.surface_ply_bytes(c, 0.2, gc)}
    assert {k: hashlib.sha256(x).hexdigest() for k, x in got.items()} == PLY_BEFORE
    assert got["mesh"] == MR.ply_bytes(v, tri) and got["surface"] == R.ply_bytes(c, 0.2)


def test_ply_with_normals(tmp_path):
    e, v, tri, c, gv, gc = _ply_inputs()
    nv, nc = N.vertex_normals(e, v)[0], N.vertex_normals(e, N.crossing_vertices(c))[0]
    assert nv.any(axis=1).sum() > 300 and nc.any(axis=1).sum() > 100
    xyz, nrm, wgt = ["property float x", "property float y", "property float z"], ["property float nx", "property float ny", "property float nz"], ["property uint weight"]
    rgb = ["property uchar red", "property uchar green", "property uchar blue"]
    for gray in (None, gv):
        data = libviso_amd.mesh_normals_ply_bytes(v, tri, nv, gray)
        head, _, body = data.partition(b"end_header\n")
        lines = head.decode("ascii").split("\n")
        assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and f"element vertex {len(v)}" in lines and f"element face {len(tri)}" in lines
        assert [ln for ln in lines if ln.startswith("property")] == xyz + nrm + wgt + (rgb if gray is not None else []) + ["property list uchar int vertex_indices"]
        size = 28 + (3 if gray is not None else 0)
        assert len(body) == size * len(v) + 13 * len(tri)
        rec = np.frombuffer(body[:size * len(v)], np.dtype([("xyz", "<f4", (3,)), ("n", "<f4", (3,)), ("weight", "<u4")] + ([("rgb", "u1", (3,))] if gray is not None else [])))
        assert _same(rec["xyz"], v["p"]) and _same(rec["n"], nv) and np.array_equal(rec["weight"], v["weight"])
        assert gray is None or (rec["rgb"] == gray[:, None]).all()
        faces = np.frombuffer(body[size * len(v):], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
        assert (faces["n"] == 3).all() and np.array_equal(faces["v"], tri)
    f = tmp_path / "m.ply"
    libviso_amd.write_mesh_normals_ply(str(f), v, tri, nv)
    assert f.read_bytes() == libviso_amd.mesh_normals_ply_bytes(v, tri, nv)
    data = libviso_amd.surface_normals_ply_bytes(c, 0.2, nc, gc)
    head, _, body = data.partition(b"end_header\n")
    assert [ln for ln in head.decode("ascii").split("\n") if ln.startswith("property")] == xyz + nrm + wgt + rgb and len(body) == 31 * len(c)
    rec = np.frombuffer(body, np.dtype([("xyz", "<f4", (3,)), ("n", "<f4", (3,)), ("weight", "<u4"), ("rgb", "u1", (3,))]))
    assert _same(rec["xyz"], R.crossing_points(c, 0.2)) and _same(rec["n"], nc) and (rec["rgb"] == gc[:, None]).all()
    f = tmp_path / "s.ply"
    libviso_amd.write_surface_normals_ply(str(f), c, 0.2, nc)
    assert f.read_bytes() == libviso_amd.surface_normals_ply_bytes(c, 0.2, nc)
    for bad in (nv[:-1], nv.astype(np.float64), nv[:, :2], None):
        with pytest.raises(ValueError):
            libviso_amd.mesh_normals_ply_bytes(v, tri, bad)


# ---- shade_normals -----------------------------------------------------------------------------------------------------------------
def test_shade_normals_on_hand_values():
    n = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.6, 0.0, -0.8], [1.0, 0.0, 0.0], [0.0, -0.6, -0.8]], np.float32)
    s = libviso_amd.shade_normals(n)
    assert s.dtype == np.uint8 and s.tolist() == [255, 0, 0, 204, 0, 204]        # 255 x 0.8 = 204.0 (float32 0.8 is above 0.8)
    assert libviso_amd.shade_normals(n, light=(0.0, 0.0, -7.5)).tolist() == s.tolist()          # a light that is not normalised
    assert libviso_amd.shade_normals(n, light=(3.0, 0.0, -4.0)).tolist() == [204, 0, 0, 255, 153, 163]   # 0.64 x 255 = 163.2
    assert libviso_amd.shade_normals(n.reshape(2, 3, 3)).shape == (2, 3)
    assert libviso_amd.shade_normals(np.zeros((0, 3), np.float32)).shape == (0,)
    for bad in (dict(normals=np.zeros((2, 2))), dict(normals=n, light=(0, 0, 0)), dict(normals=n, light=(0, np.nan, 1)), dict(normals=n, light=(1, 2))):
        with pytest.raises(ValueError):
            libviso_amd.shade_normals(**bad)


# ---- the tool's flags --------------------------------------------------------------------------------------------------------------
def test_tool_flags_need_their_modes(capsys):
    for argv in (["d", "p", "c", "o.ply", "--normals"], ["d", "p", "c", "o.ply", "--surface", "--shaded", "x"]):
        with pytest.raises(SystemExit):
            fuse_map.main(argv)
    err = capsys.readouterr().err
    assert "--normals needs --surface or --mesh" in err and "--shaded needs --render" in err
