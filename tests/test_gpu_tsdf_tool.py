"""python -m libviso_amd.fuse_map --surface on what a KITTI runner wrote with --disparity DIR: the PLY equals the restatement
(tests/tsdf_ref.py) applied to the decoded PNGs and the parsed pose file, byte for byte; without --surface the tool writes what it
wrote before the option existed (tests/map_ref.ply_bytes)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import Param

import disparity_ref as DR
import kitti_tree
import map_ref as M
import tsdf_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = "48,9,31,10,15,1"


def _run(cmd, home):
    env = dict(os.environ, KITTI_HOME=home, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_surface_mode_equals_restatement_and_plain_mode_is_unchanged(viso, tmp_path):
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
    for tag, args in (("plain", []), ("surface", ["--surface", "--capacity-log2", "22"]),
                      ("opts", ["--surface", "--capacity-log2", "22", "--voxel", "0.5", "--trunc", "2", "--min-weight", "3", "--min-disp", "2.5",
                                "--frames", "1", "4"])):
        out = os.path.join(home, tag + ".ply")
        _run([sys.executable, "-m", "libviso_amd.fuse_map", d, poses, calib, out] + args, home)
        plys[tag] = open(out, "rb").read()
    # the restatements over the decoded files
    names = sorted(os.listdir(d))
    assert names == ["%06d.png" % (first + t) for t in range(nf)]
    maps = []
    for n in names:
        v = DR.read_disparity_png(os.path.join(d, n)).astype(np.int32)
        assert (v % 16 == 0).all()
        maps.append(np.where(v == 0, M.INVALID, v // 16).astype(np.int16))
    T = []
    for line in open(poses):
        P = np.eye(4)
        P[:3] = np.array([float(x) for x in line.split()]).reshape(3, 4)
        T.append(P)
    assert len(T) == nf
    P1, P2 = seq["P1"], seq["P2"]
    rd = lambda v: float("%.12e" % v)   # noqa: E731  calib.txt carries 12 digits
    prm = Param.default(base=abs(rd(P2[0, 3]) / rd(P2[0, 0])), f=rd(P1[0, 0]), cu=rd(P1[0, 2]), cv=rd(P1[1, 2]))
    want, st = M.fuse(list(zip(maps, T)), prm, 0.2, 16)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0 and len(want) > 100
    assert plys["plain"] == M.ply_bytes(want, 0.2)
    want, st = R.fuse(list(zip(maps, T)), prm, 0.2, 3, 16, 22)
    c = R.crossings(want)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0 and len(c) > 100
    assert plys["surface"] == R.ply_bytes(c, 0.2)
    want, st = R.fuse(list(zip(maps[1:4], T[1:4])), prm, 0.5, 2, 40, 22)
    c = R.crossings(want, 3)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0 and len(c) > 10
    assert plys["opts"] == R.ply_bytes(c, 0.5)
