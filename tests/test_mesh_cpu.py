"""The triangle mesh of the TSDF map (include/viso_hip.h, "TSDF mesh") without a device: the numpy restatement (tests/mesh_ref.py)
against the properties a marching-tetrahedra mesh must have (closed, oriented, Euler characteristic, signed volume), against the
crossings of tests/tsdf_ref.py on the axis edges, on the hand-made cases of the definition (a zero sum, an incomplete cell), on the
fronto-parallel wall; the struct layout, the argument checks of the C ABI, the PLY bytes and the kernel's resource usage."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import TSDF_ENTRY_DTYPE, TSDF_MESH_VERTEX_DTYPE, Param

import mesh_ref as MR
import tsdf_ref as R
from estimator_util import kernel_resources


def _param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)


def _block(n, sums, weight=1, origin=(0, 0, 0)):
    """The voxels origin + 0 .. n-1 cubed with the sums of a function of the offset, sorted by key."""
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    e = np.zeros(len(g), TSDF_ENTRY_DTYPE)
    e["k"], e["weight"] = g + np.asarray(origin), weight
    e["sum"] = [sums(*k) for k in g.tolist()]
    return e[np.argsort(R.keys_of(e["k"]))]


def test_sphere_is_a_closed_oriented_surface_of_genus_zero():
    """The signed distance from a sphere of radius 3.7 about (5.3, 5.3, 5.3) in a block of 12^3 voxels: the data is complete around
    the surface, so the mesh is closed.  Integers only: every directed edge once and its reverse once, V - E + F = 2, and six times
    the signed volume of the midpoint mesh (the sum of v0 . (v1 x v2), in half voxels cubed) positive: the normals point out of the
    sphere, to the positive side."""
    e = MR.sphere_entries()
    assert len(e) == 12 ** 3 and (e["sum"] < 0).any() and (e["sum"] > 0).any() and (np.abs(e["sum"]) <= 3 * 1024).all()
    for weight, min_weight in ((1, 1), (3, 2)):
        v, t = MR.mesh(MR.sphere_entries(weight=weight), 0.2, min_weight)
        assert v.dtype == MR.VERTEX and t.dtype == np.uint32 and t.shape == (len(t), 3)
        assert (len(v), len(t)) == (758, 1512)
        ok, n_edges = MR.closed_and_oriented(t)
        assert ok and n_edges == 2268 and len(v) - n_edges + len(t) == 2
        m = MR.midpoints2(v)
        vol6 = int((m[t[:, 0]] * np.cross(m[t[:, 1]], m[t[:, 2]])).sum())
        print(f"sphere: {len(v)} vertices, {n_edges} edges, {len(t)} triangles, 6 x volume = {vol6} half voxels cubed")
        assert vol6 > 0
        # the interpolated mesh encloses roughly the sphere (its volume in voxels cubed; the mesh is a polyhedron inside a band)
        p = v["p"].astype(np.float64) / 0.2
        vol = (p[t[:, 0]] * np.cross(p[t[:, 1]], p[t[:, 2]])).sum() / 6.0
        assert 0.8 < vol / (4.0 / 3.0 * np.pi * 3.7 ** 3) < 1.05
        # sorted, every vertex referred to, no triangle with a repeated vertex
        assert (np.diff(R.keys_of(v["k"]) * 8 + v["dir"]) > 0).all() and len(np.unique(t)) == len(v)
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 1] != t[:, 2]).all() and (t[:, 0] != t[:, 2]).all()
        assert (v["weight"] == weight).all() and ((v["dir"] >= 1) & (v["dir"] <= 7)).all()
    assert len(MR.mesh(MR.sphere_entries(weight=3), 0.2, 4)[1]) == 0


def test_axis_vertices_are_the_crossings_bit_for_bit():
    rng = np.random.default_rng(3)
    e = _block(9, lambda x, y, z: 0)
    e = e[rng.random(len(e)) < 0.8]
    e["weight"] = rng.integers(1, 4, len(e))
    e["sum"] = (rng.integers(-3 * 1024, 3 * 1024 + 1, len(e)) * rng.integers(0, 2, len(e))) * e["weight"].astype(np.int64)
    n_axis = 0
    for voxel in (0.05, 0.2, 5.0):
        for mw in (1, 2):
            v, t = MR.mesh(e, voxel, mw)
            c = R.crossings(e, mw)
            ax = v[np.isin(v["dir"], (1, 2, 4))]
            axis = np.log2(ax["dir"]).astype(np.int64)
            # a subset of the crossings: an axis edge whose cells are all incomplete carries a crossing and no vertex
            pos = np.searchsorted(R.keys_of(c["k"]) * 3 + c["axis"], R.keys_of(ax["k"]) * 3 + axis)
            assert len(ax) <= len(c) and (pos < len(c)).all()
            hit = c[pos]
            assert np.array_equal(hit["k"], ax["k"]) and np.array_equal(hit["axis"], axis)
            assert np.array_equal(R.crossing_points(hit, voxel).view(np.uint32), ax["p"].view(np.uint32))
            assert np.array_equal(libviso_amd.tsdf_crossing_points(hit, voxel).view(np.uint32), ax["p"].view(np.uint32))
            assert np.array_equal(np.minimum(hit["wa"], hit["wb"]), ax["weight"])
            n_axis += len(ax)
    assert n_axis > 100


def test_zero_sum_gives_t_zero_and_keeps_the_degenerate_triangle():
    """One cell: corner 0 with sum 0 (positive by the rule), the seven others negative.  Every tetrahedron has corner 0 alone on its
    side: six triangles over the seven edges out of corner 0, all vertices at t = 0, the centre of voxel 0: zero area, kept."""
    e = _block(2, lambda x, y, z: 0 if (x, y, z) == (0, 0, 0) else -700)
    v, t = MR.mesh(e, 1.0)
    assert len(t) == 6 and len(v) == 7 and v["dir"].tolist() == [1, 2, 3, 4, 5, 6, 7] and (v["k"] == 0).all()
    assert (v["p"] == np.float32(0.5)).all()
    assert len({tuple(r) for r in t.tolist()}) == 6 and (np.sort(t, axis=1)[:, 0] != np.sort(t, axis=1)[:, 1]).all()
    # with the sum one unit below zero the corner joins the others: nothing
    e["sum"][0] = -1
    assert len(MR.mesh(e, 1.0)[1]) == 0
    # and one unit above: the same six triangles with area
    e["sum"][0] = 1
    v2, t2 = MR.mesh(e, 1.0)
    assert np.array_equal(t2, t) and (v2["p"] > np.float32(0.5)).any()


def test_incomplete_cell_emits_nothing_and_its_neighbours_keep_the_shared_vertices():
    """A plane x = 1.4 through a 3 x 3 x 3 block (eight cells), then the same with voxel (2, 2, 2) removed, then with it under
    min_weight: only the cell of voxel (1, 1, 1) has it as a corner, so that cell's triangles go and all others stay, with the
    vertices they share with it."""
    plane = lambda x, y, z: int((1.4 - x) * 1024)          # noqa: E731
    e = _block(3, plane, weight=2)
    v, t = MR.mesh(e, 0.2)
    # the plane cuts the four cells at x = 1 (between x = 1 and x = 2): 6 tetrahedra a cell
    assert len(t) == 4 * 8 and set(np.unique(v["k"][:, 0]).tolist()) == {1}
    for variant in ("missing", "light"):
        f = e.copy()
        i = int(np.nonzero((f["k"] == 2).all(axis=1))[0][0])
        if variant == "missing":
            f = np.delete(f, i)
            v1, t1 = MR.mesh(f, 0.2)
        else:
            f["weight"][i], f["sum"][i] = 1, f["sum"][i] // 2
            v1, t1 = MR.mesh(f, 0.2, 2)
            assert len(MR.mesh(f, 0.2, 1)[1]) == len(t)
        assert len(t1) == 3 * 8
        # the other cells' triangles, by position, are those of the whole block without the cell of (1, 1, 1)
        whole = {tuple(map(tuple, v["p"][r].tolist())) for r in t.tolist()}
        rest = {tuple(map(tuple, v1["p"][r].tolist())) for r in t1.tolist()}
        assert rest < whole and len(whole) == len(t) and len(rest) == len(t1)
        # the vertices on the cell's faces towards its neighbours are still there: owners (1, 1, 1) with dir 1 (an edge of three
        # other cells too), but no edge that only the dropped cell has (its diagonal, dir 7 from (1, 1, 1))
        own = v1[(v1["k"] == 1).all(axis=1)]
        assert 1 in own["dir"].tolist() and 7 not in own["dir"].tolist()
        assert 7 in v[(v["k"] == 1).all(axis=1)]["dir"].tolist()
    # the last voxel of an axis has no cell: a block pushed against 2^20 - 1 loses nothing else
    top = _block(3, plane, weight=2, origin=(R.BIAS - 3,) * 3)
    vt, tt = MR.mesh(top, 0.2)
    assert np.array_equal(tt, t) and np.array_equal(vt["k"], v["k"] + (R.BIAS - 3)) and np.array_equal(vt["dir"], v["dir"])


@pytest.mark.parametrize("d16", [325, 115])
@pytest.mark.parametrize("voxel", [0.2, 0.05])
def test_fronto_parallel_wall_faces_the_camera(d16, voxel):
    """The wall of test_tsdf_cpu.test_fronto_parallel_wall: a constant map without a pose, seen from the origin along +z.  The
    positive side is the camera's, so every triangle's normal has z < 0.  (Normals in double from the float32 positions; a triangle
    counts as degenerate when that normal is exactly zero.)"""
    e, st = R.fuse([(np.full((37, 333), d16, np.int16), None)], _param(), voxel, 3, 16)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0
    v, t = MR.mesh(e, voxel)
    p = v["p"].astype(np.float64)
    n = np.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]])
    full = (n != 0).any(axis=1)
    print(f"disp16 {d16}, voxel {voxel}: {len(e)} voxels, {len(v)} vertices, {len(t)} triangles, {int(full.sum())} with area")
    assert full.sum() > 1000 and (n[full][:, 2] < 0).all()
    # and the surface is where the crossings put it: within 2 s of the wall (test_tsdf_cpu), plus the rounding to float32
    Z0 = _param().f * _param().base / (d16 / 16.0)
    assert (np.abs(p[:, 2] - Z0) <= 2.0 * voxel / 1024.0 + np.abs(p[:, 2]) * 2.0 ** -24).all()


def test_struct_layout():
    assert MR.VERTEX == TSDF_MESH_VERTEX_DTYPE and TSDF_MESH_VERTEX_DTYPE.itemsize == 32
    assert [TSDF_MESH_VERTEX_DTYPE.fields[n][1] for n in ("k", "dir", "p", "weight")] == [0, 12, 16, 28]
    assert libviso_amd.TSDF_MESH_VERTEX_DTYPE is TSDF_MESH_VERTEX_DTYPE


def test_argument_errors_without_a_device():
    """A handle that is not a TSDF map: both calls answer with VISO_ERR_ARG and follow no pointer.  (The checks behind a live handle,
    min_weight 0 and null outputs, are in test_gpu_mesh: only a device makes a live handle.)"""
    L = libviso_amd.load()
    nv, nt = C.c_size_t(7), C.c_size_t(7)
    v = np.zeros(1, TSDF_MESH_VERTEX_DTYPE)
    t = np.zeros((1, 3), np.uint32)
    for handle in (None, C.c_void_p(4096)):
        assert L.viso_tsdf_mesh_count(handle, 1, C.byref(nv), C.byref(nt)) == -1
        assert b"viso_tsdf_mesh_count" in L.viso_last_error()
        assert L.viso_tsdf_mesh(handle, 1, v.ctypes.data, 1, t.ctypes.data, 1, C.byref(nv), C.byref(nt)) == -1
        assert b"viso_tsdf_mesh:" in L.viso_last_error()
        assert L.viso_tsdf_mesh(handle, 0, None, 1, None, 1, None, None) == -1 and L.viso_tsdf_mesh_count(handle, 0, None, None) == -1
    assert (nv.value, nt.value) == (7, 7) and not v["weight"].any() and not t.any()


def test_ply_header_and_bytes(tmp_path):
    v, t = MR.mesh(MR.sphere_entries(weight=2), 0.2)
    data = MR.ply_bytes(v, t)
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    assert [ln for ln in lines if ln.startswith(("element", "property"))] == [
        f"element vertex {len(v)}", "property float x", "property float y", "property float z", "property uint weight",
        f"element face {len(t)}", "property list uchar int vertex_indices"]
    assert len(body) == 16 * len(v) + 13 * len(t)
    pv = np.frombuffer(body[:16 * len(v)], np.dtype([("xyz", "<f4", (3,)), ("weight", "<u4")]))
    pf = np.frombuffer(body[16 * len(v):], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert np.array_equal(pv["xyz"], v["p"]) and np.array_equal(pv["weight"], v["weight"]) and (pf["n"] == 3).all() and np.array_equal(pf["v"], t)
    assert libviso_amd.mesh_ply_bytes(v, t) == data
    f = tmp_path / "m.ply"
    libviso_amd.write_mesh_ply(str(f), v, t)
    assert f.read_bytes() == data
    empty = libviso_amd.mesh_ply_bytes(v[:0], t[:0])
    assert empty == MR.ply_bytes(v[:0], t[:0]) and b"element vertex 0\n" in empty and empty.endswith(b"end_header\n")
    with pytest.raises(ValueError):
        libviso_amd.mesh_ply_bytes(v[:5], t)


def test_tool_refuses_mesh_together_with_surface(capsys):
    from libviso_amd import fuse_map
    with pytest.raises(SystemExit) as ex:
        fuse_map.main(["maps", "poses.txt", "calib.txt", "out.ply", "--surface", "--mesh"])
    assert ex.value.code == 2 and "not allowed with" in capsys.readouterr().err


def test_mesh_kernel_has_no_scratch():
    res = kernel_resources("tsdf.hip", ("tsdf_mesh_kernel",))
    occ, scratch = res["tsdf_mesh_kernel"]
    print(f"tsdf_mesh_kernel: occupancy {occ}, scratch {scratch}")
    assert scratch == 0 and occ >= 1


def test_mesh_fails_loudly_without_a_map():
    """No device: no map can be made (VISO_ERR_HIP), and TsdfMap.mesh on a handle that is not a live map raises with the code
    rather than returning an empty mesh."""
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(libviso_amd.VisoError, match="-2"):
            libviso_amd.TsdfMap(voxel=0.2, capacity_log2=10).mesh()
    m = object.__new__(libviso_amd.TsdfMap)
    m.L, m.h = libviso_amd.load(), 4096
    try:
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            m.mesh()
    finally:
        m.h = None
