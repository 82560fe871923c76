"""The KITTI runners' opt-in --disparity DIR (viso_kitti, kitti_shard; viso_kitti_set_disparity, viso_write_disparity_png): one
16-bit PNG per frame of the range equal to the direct call, directories byte-identical over ranks, chunkings and the two runners,
and pose files unchanged by the flag."""
import filecmp
import os
import subprocess
import sys

import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth

import disparity_ref as DR
import kitti_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = "48,9,31,10,15,1"


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    home = str(tmp_path_factory.mktemp("kitti"))
    first, nf = 3, 9
    seq = synth.make_image_sequence(7, nf, n_kp=600, width=400, height=150)
    kitti_tree.write_tree(home, "05", seq, first_index=first)
    return home, first, nf, seq


def _run(home, cmd, sha):
    env = dict(os.environ, KITTI_HOME=home, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return open(os.path.join(home, "results", "05", sha, "data", "05.txt"), "rb").read()


def _same_dir(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    match, mismatch, errors = filecmp.cmpfiles(a, b, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


def test_runners_write_one_map_per_frame(viso, tree):
    home, first, nf, seq = tree
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    assert os.path.exists(exe), "libviso_amd/viso_kitti is missing: run __graft_entry__.build()"
    d = lambda name: os.path.join(home, "disp_" + name)   # noqa: E731
    plain = _run(home, [exe, "off", "05", str(first)], "off")
    one = _run(home, [exe, "on", "05", str(first), "--disparity", d("one"), "--disparity-params", PARAMS], "on")
    assert one == plain   # the pose file does not change
    assert sorted(os.listdir(d("one"))) == ["%06d.png" % (first + t) for t in range(nf)]
    D, B, c, T, u, m = (int(v) for v in PARAMS.split(","))
    for t in range(nf):
        want = libviso_amd.stereo_disparity(seq["images"][t, 0], seq["images"][t, 1], num_disp=D, block=B, prefilter_cap=c,
                                            texture_threshold=T, uniqueness=u, lr_max_diff=m)
        got = DR.read_disparity_png(os.path.join(d("one"), "%06d.png" % (first + t)))
        assert np.array_equal(got, DR.kitti_png_values(want)), t
    # ranks and chunkings: byte-identical directories and pose files
    for name, extra in (("w2", ["--gpus", "2", "--same-device"]), ("w3c2", ["--gpus", "3", "--same-device", "--chunk", "2"]),
                        ("c3", ["--chunk", "3"]), ("c1", ["--chunk", "1"])):
        got = _run(home, [exe, name, "05", str(first), "--disparity", d(name), "--disparity-params", PARAMS] + extra, name)
        assert got == plain, name
        _same_dir(d("one"), d(name))
    for w in (1, 2):
        name = f"py{w}"
        got = _run(home, [sys.executable, "-m", "libviso_amd.kitti_shard", name, "05", str(first), "--gpus", str(w), "--backend",
                          "gloo", "--same-device", "--chunk", "4", "--disparity", d(name), "--disparity-params", PARAMS], name)
        assert got == plain, name
        _same_dir(d("one"), d(name))
    # the defaults, and a bad parameter list refused before any work
    _run(home, [exe, "def", "05", str(first), str(first + 2), "--disparity", d("def")], "def")
    want = libviso_amd.stereo_disparity(seq["images"][1, 0], seq["images"][1, 1])
    assert np.array_equal(DR.read_disparity_png(os.path.join(d("def"), "%06d.png" % (first + 1))), DR.kitti_png_values(want))
    env = dict(os.environ, KITTI_HOME=home)
    for bad in (["--disparity", d("bad"), "--disparity-params", "48,4,31,10,15,1"], ["--disparity-params", PARAMS],
                ["--disparity", d("bad"), "--disparity-params", "48,9"]):
        r = subprocess.run([exe, "bad", "05", str(first)] + bad, capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode != 0, bad
