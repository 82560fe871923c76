"""python -m libviso_amd.fuse_map --surface --render DIR on what a KITTI runner wrote with --disparity DIR: the PNGs read back equal
TsdfMap.render of the same maps and poses, and the PLY is what the tool writes without --render."""
import os
import sys

import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map, synth
from libviso_amd.abi import Param

import kitti_tree
from test_gpu_tsdf_tool import PARAMS, _run

pytestmark = pytest.mark.gpu


def test_rendered_views_equal_the_method(viso, tmp_path):
    home = str(tmp_path / "kitti")
    first, nf = 3, 3
    seq = synth.make_image_sequence(7, nf, n_kp=600, width=400, height=150)
    base = kitti_tree.write_tree(home, "05", seq, first_index=first)
    calib = os.path.join(base, "calib.txt")
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    assert os.path.exists(exe), "libviso_amd/viso_kitti is missing: run __graft_entry__.build()"
    d = os.path.join(home, "disp")
    _run([exe, "one", "05", str(first), "--disparity", d, "--disparity-params", PARAMS, "--gpus", "1"], home)
    poses = os.path.join(home, "results", "05", "one", "data", "05.txt")
    views, ply, plain = os.path.join(home, "views"), os.path.join(home, "s.ply"), os.path.join(home, "plain.ply")
    opts = ["--surface", "--capacity-log2", "22", "--min-weight", "2"]
    out = _run([sys.executable, "-m", "libviso_amd.fuse_map", d, poses, calib, ply] + opts + ["--render", views, "--render-depth", "35"], home)
    assert f"{nf} views rendered" in out
    _run([sys.executable, "-m", "libviso_amd.fuse_map", d, poses, calib, plain] + opts, home)
    assert open(ply, "rb").read() == open(plain, "rb").read()
    names = fuse_map.list_maps(d)
    assert names == ["%06d.png" % (first + t) for t in range(nf)] == fuse_map.list_maps(views)
    # the same through the method
    T = fuse_map.read_poses(poses)
    f, cu, cv, b = fuse_map.read_calib(calib)
    prm = Param.default(base=b, f=f, cu=cu, cv=cv)
    maps = [fuse_map.read_disparity_png(os.path.join(d, n)) for n in names]
    tsdf = libviso_amd.TsdfMap(None, capacity_log2=22)
    for m, pose in zip(maps, T):
        tsdf.fuse(m, prm, pose=pose)
    want = tsdf.render(prm, maps[0].shape, T, max_depth=35.0, min_weight=2)
    tsdf.close()
    assert want.shape == (nf,) + maps[0].shape and (want <= fuse_map.DISP_PNG_MAX).all()
    n_valid = 0
    for i, n in enumerate(names):
        got = fuse_map.read_disparity_png(os.path.join(views, n))
        assert got.dtype == np.int16 and got.tobytes() == want[i].tobytes(), n
        n_valid += int((got != fuse_map.DISP_INVALID).sum())
    print(f"{nf} views of {maps[0].shape}: {n_valid} valid pixels")
    assert n_valid > 1000
