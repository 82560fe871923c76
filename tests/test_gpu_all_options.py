"""Every option of the KITTI runners at once (viso::RunOptions, host/viso.hpp), each at a value that is not its default, so that
a field which takes another's place on its way from a front end to the batch shows: --subpixel 2, --covariance F
--covariance-sigma 0.5, --seed 3, --chunk 2, --decode-threads 2, --disparity D --disparity-method sgm --sgm-params ...,
--speckle ..., and in a second case --rectify on raw images.  Five frames: with chunk 2 two chunk seams with their halo frames,
and with two ranks one rank seam.  The pose file, the covariance file and the PNG directory are byte-identical among viso_kitti
in one process, viso_kitti --gpus 2 and kitti_shard --gpus 2 --chunk 3; the PNGs are the direct calls' stereo_sgm +
filter_speckles of the same images, and the covariance file is Batch.covariances() under the same options."""
import os
import subprocess
import sys

import numpy as np
import pytest

import libviso_amd
from libviso_amd import kitti_shard, synth
from libviso_amd.abi import MatchParams, Param

import kitti_tree
import rectify_ref as RR
import sgm_ref as SR
from test_gpu_disparity_runner import ROOT, _same_dir
from test_gpu_sgm_runner import PARAMS as SGM_PARAMS
from test_gpu_speckle_runner import SPECKLE

pytestmark = pytest.mark.gpu

FIRST, NF, SEED, SIGMA = 3, 5, 3, 0.5


@pytest.fixture(scope="module")
def frames():
    """Five rectified frames, and the raw ones a distorted rig would have taken of them, with its calibration."""
    seq = synth.make_subpixel_image_sequence(21, NF, n_kp=1500, width=720, height=240)
    calib = synth.raw_stereo_calib(6, raw_shape=(300, 830), out_shape=(240, 720))
    return seq, synth.distort_image_sequence(seq, calib, seed=2)["images"], calib


def _cov_lines(data):
    return [[float(v) for v in line.split()] for line in data.decode().splitlines()]


@pytest.mark.parametrize("rectify", (False, True))
def test_every_option_at_once(viso, frames, tmp_path, rectify):
    seq, raw, calib = frames
    home = str(tmp_path)
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    assert os.path.exists(exe), "libviso_amd/viso_kitti is missing: run __graft_entry__.build()"
    base = kitti_tree.write_tree(home, "05", dict(seq, images=raw) if rectify else seq, first_index=FIRST)
    opts = []
    if rectify:
        os.remove(os.path.join(base, "calib.txt"))                # --rectify reads calib_cam_to_cam.txt in its place
        opts = ["--rectify", RR.write_cam_to_cam(os.path.join(home, "calib_cam_to_cam.txt"), calib)]
    env = dict(os.environ, KITTI_HOME=home, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(name, front_end, extra):
        d, cov = os.path.join(home, "maps_" + name), os.path.join(home, "cov_" + name + ".txt")
        cmd = front_end + [name, "05", str(FIRST)] + extra + opts + [
            "--subpixel", "2", "--covariance", cov, "--covariance-sigma", str(SIGMA), "--seed", str(SEED), "--decode-threads", "2",
            "--disparity", d, "--disparity-method", "sgm", "--sgm-params", SGM_PARAMS, "--speckle", "%d,%d" % SPECKLE]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stdout + r.stderr
        return open(os.path.join(home, "results", "05", name, "data", "05.txt"), "rb").read(), open(cov, "rb").read(), d

    poses, cov, maps = run("one", [exe], ["--chunk", "2"])
    assert len(poses.splitlines()) >= NF - 1 and len(cov.splitlines()) == NF - 1
    for name, front_end, extra in (("w2", [exe], ["--chunk", "2", "--gpus", "2", "--same-device"]),
                                   ("py2", [sys.executable, "-m", "libviso_amd.kitti_shard"],
                                    ["--chunk", "3", "--gpus", "2", "--backend", "gloo", "--same-device"])):
        p, c, d = run(name, front_end, extra)
        assert p == poses and c == cov, name
        _same_dir(maps, d)

    # the maps: the direct calls on the images the batch matched (rectified on the device like the batch's own)
    images = seq["images"]
    P1, P2 = seq["P1"], seq["P2"]
    if rectify:
        cal = kitti_shard.load_cam_to_cam(opts[1])
        rmaps = [libviso_amd.rectify_map(cal["K"][s], cal["D"][s], cal["R"][s], cal["P"][s], cal["out_shape"]) for s in (0, 1)]
        images = np.stack([libviso_amd.rectify_images(raw[:, s], *rmaps[s], cal["out_shape"]) for s in (0, 1)], 1)
        P1, P2 = cal["P"]
    D, p1, p2, paths, u, m = (int(v) for v in SGM_PARAMS.split(","))
    assert sorted(os.listdir(maps)) == ["%06d.png" % (FIRST + t) for t in range(NF)]
    for t in range(NF):
        sgm = libviso_amd.stereo_sgm(images[t, 0], images[t, 1], num_disp=D, p1=p1, p2=p2, paths=paths, uniqueness=u, lr_max_diff=m)
        want = libviso_amd.filter_speckles(sgm, max_size=SPECKLE[0], max_diff=SPECKLE[1])
        assert np.array_equal(SR.read_disparity_png(os.path.join(maps, "%06d.png" % (FIRST + t))), SR.kitti_png_values(want)), t

    # the covariance file: the batch API under the same sub-pixel mode, covariance mode and sigma, seed and first frame
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, NF, 1200)
    b.upload_images_only(images)
    b.detect(n_features=1200, nbinx=24, nbiny=5)
    param = Param.default(base=abs(P2[0, 3] / P2[0, 0]), f=P1[0, 0], cu=P1[0, 2], cv=P1[1, 2])
    b.set_params(MatchParams.stereo(libviso_amd.F_from_P(P1, P2)), MatchParams.temporal(), param, seed=SEED, first_frame=FIRST)
    b.set_subpixel(2)
    b.set_covariance(2, SIGMA)
    b.run_images()
    recs = b.covariances()
    b.close(); ctx.close()
    iu = np.triu_indices(6)
    # not vacuous: test_gpu_rectify.py asks for at most two failed pairs in eleven frames of this sequence
    assert (recs["status"][1:] == 1).sum() >= NF - 3
    for t, line in zip(range(1, NF), _cov_lines(cov)):
        c = recs[t]
        assert line == [float(c["status"]), float(c["n"]), float(c["sigma2"]), float(c["gap"])] + [float(v) for v in c["cov"][iu]], t
