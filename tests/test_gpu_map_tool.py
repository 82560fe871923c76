"""python -m libviso_amd.fuse_map on what a KITTI runner wrote with --disparity DIR: the PLY equals the restatement
(tests/map_ref.py) applied to the decoded PNGs and the parsed pose file, byte for byte, and is byte-identical for directories
written by one rank and by two."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = "48,9,31,10,15,1"


def _run(cmd, home):
    env = dict(os.environ, KITTI_HOME=home, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_tool_equals_restatement_and_is_rank_independent(viso, tmp_path):
    home = str(tmp_path / "kitti")
    first, nf = 3, 7
    seq = synth.make_image_sequence(7, nf, n_kp=600, width=400, height=150)
    base = kitti_tree.write_tree(home, "05", seq, first_index=first)
    calib = os.path.join(base, "calib.txt")
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    assert os.path.exists(exe), "libviso_amd/viso_kitti is missing: run __graft_entry__.build()"
    plys = {}
    for name, extra in (("one", ["--gpus", "1"]), ("two", ["--gpus", "2", "--same-device"])):
        d = os.path.join(home, "disp_" + name)
        _run([exe, name, "05", str(first), "--disparity", d, "--disparity-params", PARAMS] + extra, home)
        poses = os.path.join(home, "results", "05", name, "data", "05.txt")
        for tag, args in (("all", []), ("opts", ["--voxel", "0.5", "--min-count", "2", "--min-disp", "2.5", "--frames", "1", "5"])):
            out = os.path.join(home, f"{name}_{tag}.ply")
            _run([sys.executable, "-m", "libviso_amd.fuse_map", d, poses, calib, out] + args, home)
            plys[name, tag] = open(out, "rb").read()
    assert plys["one", "all"] == plys["two", "all"] and plys["one", "opts"] == plys["two", "opts"]
    # the restatement over the decoded files
    d = os.path.join(home, "disp_one")
    names = sorted(os.listdir(d))
    assert names == ["%06d.png" % (first + t) for t in range(nf)]
    maps = []
    for n in names:
        v = DR.read_disparity_png(os.path.join(d, n)).astype(np.int32)
        assert (v % 16 == 0).all()
        maps.append(np.where(v == 0, M.INVALID, v // 16).astype(np.int16))
    T = []
    for line in open(os.path.join(home, "results", "05", "one", "data", "05.txt")):
        P = np.eye(4)
        P[:3] = np.array([float(x) for x in line.split()]).reshape(3, 4)
        T.append(P)
    assert len(T) == nf
    P1, P2 = seq["P1"], seq["P2"]
    rd = lambda v: float("%.12e" % v)   # noqa: E731  calib.txt carries 12 digits
    prm = Param.default(base=abs(rd(P2[0, 3]) / rd(P2[0, 0])), f=rd(P1[0, 0]), cu=rd(P1[0, 2]), cv=rd(P1[1, 2]))
    want, st = M.fuse(list(zip(maps, T)), prm, 0.2, 16)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0 and len(want) > 100
    assert plys["one", "all"] == M.ply_bytes(want, 0.2)
    want, st = M.fuse(list(zip(maps[1:5], T[1:5])), prm, 0.5, 40, min_count=2)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0 and len(want) > 10
    assert plys["one", "opts"] == M.ply_bytes(want, 0.5)
    # a directory and a pose file that disagree are refused
    env = dict(os.environ, PYTHONPATH=ROOT)
    short = tmp_path / "short.txt"
    short.write_text("1 0 0 0 0 1 0 0 0 0 1 0\n")
    r = subprocess.run([sys.executable, "-m", "libviso_amd.fuse_map", d, str(short), calib, str(tmp_path / "x.ply")], capture_output=True,
                       text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode != 0 and "poses" in r.stderr
