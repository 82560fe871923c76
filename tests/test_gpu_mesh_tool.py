"""python -m libviso_amd.fuse_map --mesh on what a KITTI runner wrote with --disparity DIR: the PLY equals the restatements
(tests/tsdf_ref.py, tests/mesh_ref.py) applied to the decoded PNGs and the parsed pose file, byte for byte; without --mesh the tool
writes what it wrote before the option existed (tests/map_ref.ply_bytes, tests/tsdf_ref.ply_bytes)."""
import os
import sys

import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import Param

import disparity_ref as DR
import kitti_tree
import map_ref as M
import mesh_ref as MR
import tsdf_ref as R
from test_gpu_tsdf_tool import PARAMS, _run

pytestmark = pytest.mark.gpu


def test_mesh_mode_equals_restatement_and_the_other_modes_are_unchanged(viso, tmp_path):
    home = str(tmp_path / "kitti")
    first, nf = 3, 5
    seq = synth.make_image_sequence(7, nf, n_kp=600, width=400, height=150)
    base = kitti_tree.write_tree(home, "05", seq, first_index=first)
    calib = os.path.join(base, "calib.txt")
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    assert os.path.exists(exe), "libviso_amd/viso_kitti is missing: run __graft_entry__.build()"
    d = os.path.join(home, "disp")
    _run([exe, "one", "05", str(first), "--disparity", d, "--disparity-params", PARAMS, "--gpus", "1"], home)
    poses = os.path.join(home, "results", "05", "one", "data", "05.txt")
    plys = {}
    opts = ["--capacity-log2", "22", "--voxel", "0.5", "--trunc", "2", "--min-weight", "2", "--min-disp", "2.5", "--frames", "1", "4"]
    for tag, args in (("plain", []), ("surface", ["--surface", "--capacity-log2", "22"]), ("opts", ["--mesh"] + opts)):
        out = os.path.join(home, tag + ".ply")
        stdout = _run([sys.executable, "-m", "libviso_amd.fuse_map", d, poses, calib, out] + args, home)
        assert ("triangles" in stdout) == (tag == "opts")
        plys[tag] = open(out, "rb").read()
    names = sorted(os.listdir(d))
    maps = []
    for n in names:
        v = DR.read_disparity_png(os.path.join(d, n)).astype(np.int32)
        maps.append(np.where(v == 0, M.INVALID, v // 16).astype(np.int16))
    T = []
    for line in open(poses):
        P = np.eye(4)
        P[:3] = np.array([float(x) for x in line.split()]).reshape(3, 4)
        T.append(P)
    assert len(T) == nf == len(maps)
    P1, P2 = seq["P1"], seq["P2"]
    rd = lambda v: float("%.12e" % v)   # noqa: E731  calib.txt carries 12 digits
    prm = Param.default(base=abs(rd(P2[0, 3]) / rd(P2[0, 0])), f=rd(P1[0, 0]), cu=rd(P1[0, 2]), cv=rd(P1[1, 2]))
    want, st = M.fuse(list(zip(maps, T)), prm, 0.2, 16)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0 and plys["plain"] == M.ply_bytes(want, 0.2)
    want, st = R.fuse(list(zip(maps, T)), prm, 0.2, 3, 16, 22)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0 and plys["surface"] == R.ply_bytes(R.crossings(want), 0.2)
    want, st = R.fuse(list(zip(maps[1:4], T[1:4])), prm, 0.5, 2, 40, 22)
    v, t = MR.mesh(want, 0.5, 2)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0 and len(t) > 10 and plys["opts"] == MR.ply_bytes(v, t)
