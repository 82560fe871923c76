"""python -m libviso_amd.fuse_map --normals and --shaded DIR: the PLY carries TsdfMap.normals.vertices of the same map, the shaded
PNGs are shade_normals of TsdfMap.normals.render, and without the two flags every output is byte for byte what it is with
the flags absent.  The tool runs in this process (fuse_map.main) on maps, poses and a calibration written here."""
import os

import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map

import render_ref as RR
from test_gpu_render import _param
from test_gpu_tsdf import POSE

pytestmark = pytest.mark.gpu

SHAPE = (37, 333)


def _inputs(home):
    """Three maps of the render tests' scenes with their poses and the calibration, as a KITTI runner leaves them."""
    prm = _param()
    d = os.path.join(home, "disp")
    os.makedirs(d)
    poses = [POSE, RR.sideways(POSE, 0.05, 0.004), RR.sideways(POSE, -0.04, -0.003)]
    for i, name in enumerate(("plane", "step", "wall")):
        fuse_map.write_disparity_png(os.path.join(d, "%06d.png" % (i + 4)), RR.scene_map(name, SHAPE, 0.1))
    fuse_map.write_poses(os.path.join(home, "poses.txt"), poses)
    with open(os.path.join(home, "calib.txt"), "w") as f:
        for name, tx in (("P0", 0.0), ("P1", -prm.f * prm.base)):
            f.write(f"{name}: " + " ".join("%.17g" % v for v in (prm.f, 0, prm.cu, tx, 0, prm.f, prm.cv, 0, 0, 0, 1, 0)) + "\n")
    got = fuse_map.read_calib(os.path.join(home, "calib.txt"))
    assert got[:3] == (prm.f, prm.cu, prm.cv) and abs(got[3] - prm.base) < 1e-15
    return d, os.path.join(home, "poses.txt"), os.path.join(home, "calib.txt")


def _tool(*argv):
    assert fuse_map.main([str(a) for a in argv]) == 0


def _dir_bytes(path):
    return {n: open(os.path.join(path, n), "rb").read() for n in sorted(os.listdir(path))}


def test_normals_in_the_ply_and_shaded_views(viso, tmp_path, capsys):
    home = str(tmp_path)
    d, poses, calib = _inputs(home)
    opts = ["--capacity-log2", "20", "--min-weight", "1", "--render-depth", "20"]
    out = {k: os.path.join(home, k) for k in ("mesh.ply", "mesh_n.ply", "surf.ply", "surf_n.ply", "v0", "v1", "v2", "lit")}
    _tool(d, poses, calib, out["mesh.ply"], "--mesh", "--render", out["v0"], *opts)
    _tool(d, poses, calib, out["mesh_n.ply"], "--mesh", "--normals", "--render", out["v1"], "--shaded", out["lit"], *opts)
    _tool(d, poses, calib, out["surf.ply"], "--surface", *opts)
    _tool(d, poses, calib, out["surf_n.ply"], "--surface", "--normals", "--render", out["v2"], *opts)
    capsys.readouterr()
    # the same through the methods
    T = fuse_map.read_poses(poses)
    f, cu, cv, b = fuse_map.read_calib(calib)
    prm = libviso_amd.abi.Param.default(base=b, f=f, cu=cu, cv=cv)
    names = fuse_map.list_maps(d)
    tsdf = libviso_amd.TsdfMap(None, capacity_log2=20)
    for n, pose in zip(names, T):
        tsdf.fuse(fuse_map.read_disparity_png(os.path.join(d, n)), prm, pose=pose)
    v, tri, nv = tsdf.normals.mesh(1)
    c, nc = tsdf.surface(1), tsdf.normals.surface(1)
    views, nrm = tsdf.normals.render(prm, SHAPE, T, max_depth=20.0, min_weight=1)
    tsdf.close()
    assert nv.any(axis=1).sum() > 300 and nc.any(axis=1).sum() > 200 and nrm.any(axis=-1).sum() > 10000
    # the PLYs: with --normals the vertex normals of the same map, without it today's bytes
    assert open(out["mesh_n.ply"], "rb").read() == libviso_amd.mesh_normals_ply_bytes(v, tri, nv)
    assert open(out["surf_n.ply"], "rb").read() == libviso_amd.surface_normals_ply_bytes(c, 0.2, nc)
    assert open(out["mesh.ply"], "rb").read() == libviso_amd.mesh_ply_bytes(v, tri)
    assert open(out["surf.ply"], "rb").read() == libviso_amd.surface_ply_bytes(c, 0.2)
    heads = [open(out[k], "rb").read().partition(b"end_header")[0] for k in ("mesh_n.ply", "mesh.ply")]
    assert b"property float nx" in heads[0] and b"nx" not in heads[1]
    # the views: the flags change none of the rendered maps, and the shaded ones are shade_normals of the render
    assert _dir_bytes(out["v0"]) == _dir_bytes(out["v1"]) == _dir_bytes(out["v2"]) and sorted(_dir_bytes(out["v0"])) == names
    assert not os.path.exists(os.path.join(home, "v0", "gray")) and fuse_map.list_maps(out["lit"]) == names
    assert (views <= fuse_map.DISP_PNG_MAX).all()
    lit = libviso_amd.shade_normals(nrm)
    assert lit.dtype == np.uint8 and len(np.unique(lit)) > 3
    for i, n in enumerate(names):
        assert fuse_map.read_disparity_png(os.path.join(out["v1"], n)).tobytes() == views[i].tobytes(), n
        got = fuse_map.read_png8(os.path.join(out["lit"], n))
        assert got.shape == SHAPE and got.tobytes() == lit[i].tobytes(), n

