"""The KITTI runners' --speckle SIZE,DIFF beside --disparity DIR (viso_kitti, kitti_shard; viso_kitti_set_speckle), for both
--disparity-method values: one 16-bit PNG per frame of the range equal to the filter of the direct call, directories
byte-identical over ranks, chunkings and the two runners, pose files unchanged by the flag, the directory without --speckle the
method's own, and --speckle without --disparity refused with the usage code."""
import os
import subprocess
import sys

import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth

import disparity_ref as DR
import kitti_tree
import speckle_ref as K
from test_gpu_disparity_runner import PARAMS as BM_PARAMS, ROOT, _run, _same_dir
from test_gpu_sgm_runner import PARAMS as SGM_PARAMS

pytestmark = pytest.mark.gpu

SPECKLE = (40, 12)   # max_size, max_diff


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    home = str(tmp_path_factory.mktemp("kitti_speckle"))
    first, nf = 3, 9
    seq = synth.make_image_sequence(7, nf, n_kp=600, width=400, height=150)
    kitti_tree.write_tree(home, "05", seq, first_index=first)
    return home, first, nf, seq


def _method(method):
    """(the runner's options, the direct call) of a method with the parameters of its own runner test."""
    if method == "bm":
        D, B, c, T, u, m = (int(v) for v in BM_PARAMS.split(","))
        prm = dict(num_disp=D, block=B, prefilter_cap=c, texture_threshold=T, uniqueness=u, lr_max_diff=m)
        return ["--disparity-params", BM_PARAMS], lambda a, b: libviso_amd.stereo_disparity(a, b, **prm)
    D, p1, p2, paths, u, m = (int(v) for v in SGM_PARAMS.split(","))
    prm = dict(num_disp=D, p1=p1, p2=p2, paths=paths, uniqueness=u, lr_max_diff=m)
    return ["--disparity-method", "sgm", "--sgm-params", SGM_PARAMS], lambda a, b: libviso_amd.stereo_sgm(a, b, **prm)


@pytest.mark.parametrize("method", ("bm", "sgm"))
def test_runners_write_one_filtered_map_per_frame(viso, tree, method):
    home, first, nf, seq = tree
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    assert os.path.exists(exe), "libviso_amd/viso_kitti is missing: run __graft_entry__.build()"
    opts, direct = _method(method)
    d = lambda name: os.path.join(home, f"spk_{method}_{name}")   # noqa: E731
    sha = lambda name: f"{method}_{name}"   # noqa: E731
    spk = lambda name: ["--disparity", d(name)] + opts + ["--speckle", "%d,%d" % SPECKLE]   # noqa: E731
    plain = _run(home, [exe, sha("off"), "05", str(first)], sha("off"))
    one = _run(home, [exe, sha("one"), "05", str(first)] + spk("one"), sha("one"))
    assert one == plain   # the pose file does not change
    assert sorted(os.listdir(d("one"))) == ["%06d.png" % (first + t) for t in range(nf)]
    raw = [direct(seq["images"][t, 0], seq["images"][t, 1]) for t in range(nf)]
    removed = 0
    for t in range(nf):
        want = libviso_amd.filter_speckles(raw[t], max_size=SPECKLE[0], max_diff=SPECKLE[1])
        assert np.array_equal(want, K.speckles(raw[t], *SPECKLE)), t
        got = DR.read_disparity_png(os.path.join(d("one"), "%06d.png" % (first + t)))
        assert np.array_equal(got, DR.kitti_png_values(want)), t
        removed += int((want != raw[t]).sum())
    assert removed > 0   # the filter had something to do
    # ranks and chunkings: byte-identical directories and pose files
    for name, extra in (("w1", ["--gpus", "1", "--same-device"]), ("w2", ["--gpus", "2", "--same-device"]),
                        ("w3c2", ["--gpus", "3", "--same-device", "--chunk", "2"]), ("c1", ["--chunk", "1"]), ("c2", ["--chunk", "2"]),
                        ("c3", ["--chunk", "3"]), ("c64", ["--chunk", "64"])):
        got = _run(home, [exe, sha(name), "05", str(first)] + spk(name) + extra, sha(name))
        assert got == plain, name
        _same_dir(d("one"), d(name))
    for w in (1, 2):
        name = f"py{w}"
        got = _run(home, [sys.executable, "-m", "libviso_amd.kitti_shard", sha(name), "05", str(first), "--gpus", str(w), "--backend",
                          "gloo", "--same-device", "--chunk", "4"] + spk(name), sha(name))
        assert got == plain, name
        _same_dir(d("one"), d(name))
    # without --speckle: the method's own files, from both runners; a size of 0 is valid and gives the same
    assert _run(home, [exe, sha("raw"), "05", str(first), "--disparity", d("raw")] + opts, sha("raw")) == plain
    for t in range(nf):
        got = DR.read_disparity_png(os.path.join(d("raw"), "%06d.png" % (first + t)))
        assert np.array_equal(got, DR.kitti_png_values(raw[t])), t
    _run(home, [sys.executable, "-m", "libviso_amd.kitti_shard", sha("rawpy"), "05", str(first), "--gpus", "1", "--backend", "gloo",
                "--same-device", "--disparity", d("rawpy")] + opts, sha("rawpy"))
    _same_dir(d("raw"), d("rawpy"))
    _run(home, [exe, sha("s0"), "05", str(first), "--disparity", d("s0")] + opts + ["--speckle", "0,16"], sha("s0"))
    _same_dir(d("raw"), d("s0"))


def test_bad_option_lists_are_refused(viso, tree):
    home, first, nf, seq = tree
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    env = dict(os.environ, KITTI_HOME=home, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    d = os.path.join(home, "spk_bad")
    # --speckle without --disparity, and lists that are not two integers: the usage message and its code (1; argparse's is 2)
    for bad in (["--speckle", "40,12"], ["--disparity", d, "--speckle", "40"], ["--disparity", d, "--speckle", "40,12,3"],
                ["--disparity", d, "--speckle"]):
        r = subprocess.run([exe, "bad", "05", str(first)] + bad, capture_output=True, text=True, timeout=60, env=env)
        assert r.returncode == 1 and r.stdout.startswith("usage:"), (bad, r.returncode)
        r = subprocess.run([sys.executable, "-m", "libviso_amd.kitti_shard", "bad", "05", str(first), "--gpus", "1"] + bad,
                           capture_output=True, text=True, timeout=60, env=env, cwd=ROOT)
        assert r.returncode == 2 and "usage:" in r.stderr, (bad, r.returncode)
    # values outside the ranges of include/viso_hip.h are refused before any work
    for bad in ("-1,16", "40,-1", "40,4097"):
        r = subprocess.run([exe, "bad", "05", str(first), "--disparity", d, "--speckle", bad], capture_output=True, text=True, timeout=60,
                           env=env)
        assert r.returncode == 2 and "viso_kitti_set_speckle" in r.stderr, bad
