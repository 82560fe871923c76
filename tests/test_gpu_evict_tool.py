"""python -m libviso_amd.fuse_map --window on a directory of maps in the runners' format: a table of 2^10 slots that follows the
camera gives, with its archive, the PLY of the unbounded run, byte for byte; without the window the same table fills."""
import os
import subprocess
import sys

import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map
from libviso_amd.abi import TSDF_ENTRY_DTYPE

import evict_ref as E
import tsdf_ref as R
from test_gpu_evict import WIN, _param, _window_frames

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(args, ok=True):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "libviso_amd.fuse_map"] + args, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout + r.stderr


def _tree(tmp_path):
    """The 12 maps of test_gpu_evict's windowed run as a runner would have written them, with their pose file and a calib.txt."""
    frames = _window_frames(np.random.default_rng(14))
    prm = _param()
    d = tmp_path / "disp"
    d.mkdir()
    for i, (m, _, _) in enumerate(frames):
        fuse_map.write_disparity_png(str(d / ("%06d.png" % i)), m)
    fuse_map.write_poses(str(tmp_path / "poses.txt"), [p for _, _, p in frames])
    P0 = [prm.f, 0, prm.cu, 0, 0, prm.f, prm.cv, 0, 0, 0, 1, 0]
    P1 = list(P0)
    P1[3] = -prm.f * prm.base
    with open(tmp_path / "calib.txt", "w") as f:
        f.write("P0: " + " ".join("%.17g" % v for v in P0) + "\nP1: " + " ".join("%.17g" % v for v in P1) + "\n")
    f_, cu, cv, base = fuse_map.read_calib(str(tmp_path / "calib.txt"))
    # (the base comes back through a division: the restatements below use what the tool reads)
    return frames, type(prm).default(base=base, f=f_, cu=cu, cv=cv), [str(d), str(tmp_path / "poses.txt"), str(tmp_path / "calib.txt")]


def test_window_centroids_equal_the_unbounded_run(viso, tmp_path):
    frames, prm, inputs = _tree(tmp_path)
    w = WIN["map"]
    opts = ["--voxel", str(w["voxel"]), "--min-disp", str(w["min_disp16"] / 16)]
    whole, small, arch = (str(tmp_path / n) for n in ("whole.ply", "small.ply", "archive.npy"))
    _tool(inputs + [whole] + opts)
    out = _tool(inputs + [small] + opts + ["--capacity-log2", "10", "--window", str(w["half"]), "--archive", arch])
    assert "evicted" in out
    assert open(whole, "rb").read() == open(small, "rb").read()
    a = np.load(arch)
    assert a.dtype == libviso_amd.MAP_ENTRY_DTYPE and len(a) > 1024 and (np.diff(E.keys_of(a["k"])) > 0).all()
    # without the window the small table fills
    out = _tool(inputs + [small] + opts + ["--capacity-log2", "10"], ok=False)
    assert "slots is full" in out


def test_window_surface_archive_and_live_window_are_the_unbounded_map(viso, tmp_path):
    frames, prm, inputs = _tree(tmp_path)
    w = WIN["tsdf"]
    opts = ["--surface", "--voxel", str(w["voxel"]), "--min-disp", str(w["min_disp16"] / 16)]
    whole, small, arch = (str(tmp_path / n) for n in ("whole.ply", "small.ply", "archive.npy"))
    _tool(inputs + [whole] + opts + ["--capacity-log2", "14"])
    _tool(inputs + [small] + opts + ["--capacity-log2", "10", "--window", str(w["half"]), "--archive", arch])
    a = np.load(arch)
    assert a.dtype == TSDF_ENTRY_DTYPE and len(a) > 1024 and (np.diff(E.keys_of(a["k"])) > 0).all()
    # the same windowed run through the interface: its evicted voxels are the tool's archive, its live ones the tool's window
    tsdf = libviso_amd.TsdfMap(None, voxel=w["voxel"], min_disp16=w["min_disp16"], capacity_log2=10)
    gone = []
    for m, _, pose in frames:
        gone.append(tsdf.evict(libviso_amd.voxel_box(pose[:3, 3], w["half"], w["voxel"])))
        tsdf.fuse(m, prm, pose=pose)
    live = tsdf.entries()
    window_ply = libviso_amd.surface_ply_bytes(tsdf.surface(), w["voxel"])
    tsdf.close()
    assert a.tobytes() == R.merge(*gone).tobytes()
    assert open(small, "rb").read() == window_ply                                   # OUT.ply: the live window
    full = libviso_amd.TsdfMap(None, voxel=w["voxel"], min_disp16=w["min_disp16"], capacity_log2=14)
    full.add_entries(libviso_amd.merge_entries(a, live))
    ply = libviso_amd.surface_ply_bytes(full.surface(), w["voxel"])
    full.close()
    assert ply == open(whole, "rb").read() and len(ply) > len(window_ply)
