"""The KITTI runners' --disparity DIR --disparity-method sgm [--sgm-params ...] (viso_kitti, kitti_shard; viso_kitti_set_sgm): one
16-bit PNG per frame of the range equal to the direct call, directories byte-identical over ranks, chunkings and the two runners,
pose files unchanged by the flag, and --disparity-method bm / no method the block matcher's files byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth

import kitti_tree
import sgm_ref as SR
from test_gpu_disparity_runner import PARAMS as BM_PARAMS, _run, _same_dir

pytestmark = pytest.mark.gpu

PARAMS = "48,7,86,8,10,1"


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    home = str(tmp_path_factory.mktemp("kitti_sgm"))
    first, nf = 3, 9
    seq = synth.make_image_sequence(7, nf, n_kp=600, width=400, height=150)
    kitti_tree.write_tree(home, "05", seq, first_index=first)
    return home, first, nf, seq


def test_runners_write_one_sgm_map_per_frame(viso, tree):
    home, first, nf, seq = tree
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    assert os.path.exists(exe), "libviso_amd/viso_kitti is missing: run __graft_entry__.build()"
    d = lambda name: os.path.join(home, "sgm_" + name)   # noqa: E731
    sgm = lambda name: ["--disparity", d(name), "--disparity-method", "sgm", "--sgm-params", PARAMS]   # noqa: E731
    plain = _run(home, [exe, "off", "05", str(first)], "off")
    one = _run(home, [exe, "on", "05", str(first)] + sgm("one"), "on")
    assert one == plain   # the pose file does not change
    assert sorted(os.listdir(d("one"))) == ["%06d.png" % (first + t) for t in range(nf)]
    D, p1, p2, paths, u, m = (int(v) for v in PARAMS.split(","))
    prm = dict(num_disp=D, p1=p1, p2=p2, paths=paths, uniqueness=u, lr_max_diff=m)
    for t in range(nf):
        want = libviso_amd.stereo_sgm(seq["images"][t, 0], seq["images"][t, 1], **prm)
        got = SR.read_disparity_png(os.path.join(d("one"), "%06d.png" % (first + t)))
        assert np.array_equal(got, SR.kitti_png_values(want)), t
    assert np.array_equal(libviso_amd.stereo_sgm(seq["images"][4, 0], seq["images"][4, 1], **prm), SR.sgm(seq["images"][4, 0], seq["images"][4, 1], **prm))
    # ranks and chunkings: byte-identical directories and pose files
    for name, extra in (("w2", ["--gpus", "2", "--same-device"]), ("w3c2", ["--gpus", "3", "--same-device", "--chunk", "2"]),
                        ("c3", ["--chunk", "3"]), ("c1", ["--chunk", "1"])):
        got = _run(home, [exe, name, "05", str(first)] + sgm(name) + extra, name)
        assert got == plain, name
        _same_dir(d("one"), d(name))
    for w in (1, 2):
        name = f"py{w}"
        got = _run(home, [sys.executable, "-m", "libviso_amd.kitti_shard", name, "05", str(first), "--gpus", str(w), "--backend",
                          "gloo", "--same-device", "--chunk", "4"] + sgm(name), name)
        assert got == plain, name
        _same_dir(d("one"), d(name))
    # the defaults
    _run(home, [exe, "def", "05", str(first), str(first + 2), "--disparity", d("def"), "--disparity-method", "sgm"], "def")
    want = libviso_amd.stereo_sgm(seq["images"][1, 0], seq["images"][1, 1])
    assert np.array_equal(SR.read_disparity_png(os.path.join(d("def"), "%06d.png" % (first + 1))), SR.kitti_png_values(want))
    # --disparity-method bm and no method: the block matcher's files, byte for byte, from both runners
    bm = ["--disparity-params", BM_PARAMS]
    assert _run(home, [exe, "bm0", "05", str(first), "--disparity", d("bm0")] + bm, "bm0") == plain
    assert _run(home, [exe, "bm1", "05", str(first), "--disparity", d("bm1"), "--disparity-method", "bm"] + bm, "bm1") == plain
    _same_dir(d("bm0"), d("bm1"))
    _run(home, [sys.executable, "-m", "libviso_amd.kitti_shard", "bm2", "05", str(first), "--gpus", "1", "--backend", "gloo",
                "--same-device", "--disparity", d("bm2"), "--disparity-method", "bm"] + bm, "bm2")
    _same_dir(d("bm0"), d("bm2"))
    Db, B, c, T, ub, mb = (int(v) for v in BM_PARAMS.split(","))
    want = libviso_amd.stereo_disparity(seq["images"][2, 0], seq["images"][2, 1], num_disp=Db, block=B, prefilter_cap=c,
                                        texture_threshold=T, uniqueness=ub, lr_max_diff=mb)
    assert np.array_equal(SR.read_disparity_png(os.path.join(d("bm0"), "%06d.png" % (first + 2))), SR.kitti_png_values(want))
    # bad option lists are refused before any work
    env = dict(os.environ, KITTI_HOME=home)
    for bad in (["--disparity", d("bad"), "--disparity-method", "sgm", "--sgm-params", "48,7,86,6,10,1"],
                ["--disparity", d("bad"), "--disparity-method", "sgm", "--sgm-params", "48,7"],
                ["--disparity", d("bad"), "--disparity-method", "census"],
                ["--disparity", d("bad"), "--sgm-params", PARAMS],
                ["--disparity", d("bad"), "--disparity-method", "sgm", "--disparity-params", BM_PARAMS],
                ["--disparity-method", "sgm"]):
        r = subprocess.run([exe, "bad", "05", str(first)] + bad, capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode != 0, bad
