"""The opt-in rectification of raw images on the device (include/viso_hip.h, viso_batch_set_rectify / viso_rectify_images;
libviso_amd/csrc/rectify.hip) against its numpy restatement (tests/rectify_ref.py) and the CPU-assembled pipeline."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MatchParams, Param

import rectify_ref as RR
import subpixel_ref as S
from dense_fuzz import hostile_map as _hostile_map

pytestmark = pytest.mark.gpu

# Medians of the CPU assembly of test_rectification_restores_accuracy's scene (same arithmetic as the device): 15.1 mm on the
# original rectified images, 13.0 mm rectified from raw, 383 mm on the raw images unrectified.
RECT_FACTOR = 1.5
RAW_FACTOR = 5.0


@pytest.mark.parametrize("raw_shape,out_shape", [((37, 53), (29, 41)), ((9, 9), (9, 9)), ((20, 30), (43, 57)), ((512, 1392), (376, 1241))])
def test_rectify_images_bit_exact(viso, raw_shape, out_shape):
    rng = np.random.default_rng(raw_shape[0] * 1000 + out_shape[1])
    raw = rng.integers(0, 256, (3,) + raw_shape, dtype=np.uint8)
    maps = [_hostile_map(rng, raw_shape, out_shape)]
    if raw_shape == (512, 1392):
        c = synth.raw_stereo_calib(1)
        maps.append(libviso_amd.rectify_map(c["K"][1], c["D"][1], c["R"][1], c["P"][1], out_shape))
    for mx, my in maps:
        for border in (0, 200):
            got = libviso_amd.rectify_images(raw, mx, my, out_shape, border=border)
            for i in range(len(raw)):
                want = RR.remap(raw[i], mx, my, border)
                assert np.array_equal(got[i], want), (raw_shape, out_shape, border, i)
    one = libviso_amd.rectify_images(raw[1], mx, my, out_shape, border=7)
    assert np.array_equal(one, RR.remap(raw[1], mx, my, 7))


def test_batch_uploads_sync_and_async(viso):
    rng = np.random.default_rng(5)
    raw_shape, out_shape, nf, cap = (61, 83), (47, 71), 7, 64
    maps = [_hostile_map(rng, raw_shape, out_shape) for _ in range(2)]
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, nf, cap)
    b.set_rectify(raw_shape, out_shape, left=maps[0], right=maps[1], border=33)
    kp = np.zeros((nf, 2, cap, 2), np.float32)
    kp[..., 0] = rng.integers(6, out_shape[1] - 6, (nf, 2, cap)); kp[..., 1] = rng.integers(6, out_shape[0] - 6, (nf, 2, cap))
    n = np.full((nf, 2), cap, np.int32)
    b.set_params(MatchParams.stereo(libviso_amd.F_from_P(synth.KITTI_P1, synth.KITTI_P2)), MatchParams.temporal(),
                 Param.default(), seed=1)
    for rnd in range(3):
        raw = rng.integers(0, 256, (nf, 2) + raw_shape, dtype=np.uint8)
        b.upload_images(raw[:2], kp[:2], n[:2])                          # sync, f0 = 0
        b.upload_images_only(raw[2:4], f0=2)                             # sync without keypoints
        pin = libviso_amd.PinnedArray((nf - 4, 2) + raw_shape, np.uint8)
        pin.a[...] = raw[4:]
        kp_async = np.ascontiguousarray(kp[4:])                          # untouched until the stream has passed the copy
        b.upload_images_async(pin.a, kp_async, n[4:], f0=4)
        b.run_images()
        want = RR.rectify_sequence(raw, maps, border=33)
        for t in range(nf):
            for side in (0, 1):
                assert np.array_equal(b.image(t, side), want[t, side]), (rnd, t, side)
        pin.close()
    b.close(); ctx.close()


def _device_keypoints(b, nf, cap):
    kp = np.zeros((nf, 2, cap, 2), np.float32); n = np.zeros((nf, 2), np.int32)
    for t in range(nf):
        for side in range(2):
            k = b.keypoints(t, side)
            kp[t, side, :len(k)] = k; n[t, side] = len(k)
    return kp, n


@pytest.fixture(scope="module")
def raw32():
    seq = synth.make_subpixel_image_sequence(8, 32, n_kp=600, width=640, height=200)
    calib = synth.raw_stereo_calib(3, raw_shape=(250, 730), out_shape=(200, 640))
    d = synth.distort_image_sequence(seq, calib, seed=4)
    maps = RR.maps_of(calib)
    return d, maps, RR.rectify_sequence(d["images"], maps)


@pytest.mark.parametrize("detect", [False, True])
def test_batch_pipeline_against_cpu_assembly(viso, oracle, raw32, detect):
    d, maps, rect = raw32
    nf, _, cap, _ = d["kp"].shape
    ctx = libviso_amd.Context(0)
    for mode in (0, 1):
        b = libviso_amd.Batch(ctx, nf, cap)
        b.set_rectify(d["calib"]["raw_shape"], d["calib"]["out_shape"], left=maps[0], right=maps[1])
        if detect:
            b.upload_images_only(d["images"])
            b.detect(n_features=cap, nbinx=8, nbiny=3)
        else:
            b.upload_images(d["images"], d["kp"], d["n"])
        b.set_params(MatchParams.stereo(d["F"]), MatchParams.temporal(), d["param"], seed=5)
        b.set_subpixel(mode)
        b.run_images()
        for t in (0, nf // 2, nf - 1):
            assert np.array_equal(b.image(t, 0), rect[t, 0]) and np.array_equal(b.image(t, 1), rect[t, 1])
        kp, n = (_device_keypoints(b, nf, cap) if detect else (d["kp"], d["n"]))
        if detect:
            for t in (0, nf - 1):
                k0, _ = oracle.detect_harris_binned(rect[t, 0], cap, 8, 3)
                assert np.array_equal(kp[t, 0, :n[t, 0]], k0)
        want = S.pipeline(oracle, dict(d, images=rect, kp=kp, n=n), mode, seed=5)
        tr, ok, n_inl = b.poses()
        for t in range(nf):
            assert np.array_equal(b.matches(0, t), want["lr"][t]), (mode, t)
        assert np.array_equal(ok, want["ok"]) and np.array_equal(n_inl, want["n_inl"]), mode
        for t in range(1, nf):
            if ok[t]:
                a, r = libviso_amd.tr2mat(tr[t]), oracle.tr2mat(want["tr"][t])
                assert np.linalg.norm(a - r) / np.linalg.norm(r) < 1e-5
        b.close()
    ctx.close()


def test_identity_maps_change_nothing(viso):
    seq = synth.make_image_sequence(6, 8, n_kp=500, width=500, height=180)
    nf, _, cap, _ = seq["kp"].shape
    rows, cols = 180, 500
    gy, gx = np.mgrid[0:rows, 0:cols].astype(np.float32)
    ctx = libviso_amd.Context(0)

    def run(b):
        b.upload_images_only(seq["images"])
        b.detect(n_features=cap, nbinx=10, nbiny=3)
        b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=2)
        b.run_images()
        return _device_keypoints(b, nf, cap), [b.matches(w, t) for t in range(nf) for w in range(3 if t else 1)], b.poses()

    ref = libviso_amd.Batch(ctx, nf, cap)
    want = run(ref)
    b = libviso_amd.Batch(ctx, nf, cap)
    b.set_rectify((rows, cols), (rows, cols), left=(gx, gy), right=(gx, gy))
    for phase in ("identity", "off"):
        got = run(b)
        assert all(np.array_equal(x, y) for x, y in zip(got[0], want[0])), phase
        assert all(np.array_equal(x, y) for x, y in zip(got[1], want[1])), phase
        assert all(np.array_equal(x, y) for x, y in zip(got[2], want[2])), phase
        b.set_rectify(None)
    # a wrong raw geometry is refused and the batch stays usable
    b.set_rectify((rows + 2, cols), (rows, cols), left=(gx, gy), right=(gx, gy))
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.upload_images_only(seq["images"])
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.set_rectify((rows, cols), (rows, cols), left=(gx, gy), right=(gx, gy), border=300)
    b.set_rectify(None)
    got = run(b)
    assert all(np.array_equal(x, y) for x, y in zip(got[2], want[2]))
    b.close(); ref.close(); ctx.close()


def test_rectification_restores_accuracy(viso):
    """On the distorted scene the median translation error with rectification is close to the error on the original rectified
    images, and far below the error of feeding the raw images unrectified (thresholds from the CPU assembly of this scene,
    DESIGN.md "Rectification")."""
    seq = synth.make_subpixel_image_sequence(2, 12, n_kp=1500)
    calib = synth.raw_stereo_calib(5)
    d = synth.distort_image_sequence(seq, calib, seed=7)
    maps = [libviso_amd.rectify_map(calib["K"][s], calib["D"][s], calib["R"][s], calib["P"][s], calib["out_shape"]) for s in (0, 1)]
    ctx = libviso_amd.Context(0)
    err = {}
    for name in ("orig", "rect", "raw"):
        b = libviso_amd.Batch(ctx, 12, 1500)
        if name == "rect":
            b.set_rectify(calib["raw_shape"], calib["out_shape"], left=maps[0], right=maps[1])
        b.upload_images_only(seq["images"] if name == "orig" else d["images"])
        b.detect(n_features=1500, nbinx=24, nbiny=5)
        b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=3)
        b.run_images()
        tr, ok, _ = b.poses()
        err[name] = np.median(S.translation_errors(tr, seq["tr_gt"]))
        b.close()
    ctx.close()
    assert err["rect"] < RECT_FACTOR * err["orig"] and err["raw"] > RAW_FACTOR * err["rect"], err


def test_detect_after_the_geometry_grows(viso, oracle):
    """An upload of larger images reallocates the image buffer and drops the Harris response scratch sized for the old
    geometry; detection on the new images is the oracle's (rectification changes the geometry the same way)."""
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 2, 600)
    for rows, cols in ((48, 64), (200, 320), (120, 500)):
        imgs = np.stack([np.stack([synth.make_images(rows * 7 + t * 2 + s, rows, cols) for s in (0, 1)]) for t in range(2)])
        b.upload_images_only(imgs)
        assert b.image_shape() == (rows, cols)
        b.detect(n_features=600, nbinx=4, nbiny=2)
        for t in range(2):
            for s in (0, 1):
                k0, _ = oracle.detect_harris_binned(imgs[t, s], 600, 4, 2)
                assert np.array_equal(b.keypoints(t, s), k0), (rows, cols, t, s)
    b.close(); ctx.close()


def test_kitti_runners_with_rectify(viso, tmp_path):
    """A tiny raw KITTI tree with calib_cam_to_cam.txt (and no calib.txt): viso_kitti --rectify and kitti_shard --rectify write
    byte-identical pose files for one and two ranks and any chunking (a halo frame is rectified again like any other), and
    the poses are the batch API's on the same raw frames."""
    import os
    import subprocess
    import sys

    import kitti_tree
    from libviso_amd import hostmath, kitti_shard
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    home, first, nf = str(tmp_path), 3, 11
    seq = synth.make_subpixel_image_sequence(21, nf, n_kp=1500, width=720, height=240)
    calib = synth.raw_stereo_calib(6, raw_shape=(300, 830), out_shape=(240, 720))
    d = synth.distort_image_sequence(seq, calib, seed=2)
    base = kitti_tree.write_tree(home, "05", dict(seq, images=d["images"]), first_index=first)
    os.remove(os.path.join(base, "calib.txt"))                    # --rectify reads calib_cam_to_cam.txt in its place
    cc = RR.write_cam_to_cam(os.path.join(home, "calib_cam_to_cam.txt"), calib)
    env = dict(os.environ, KITTI_HOME=home, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(cmd, sha):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert r.returncode == 0, r.stdout + r.stderr
        return open(os.path.join(home, "results", "05", sha, "data", "05.txt"), "rb").read()

    one = run([exe, "r1", "05", str(first), "--rectify", cc], "r1")
    assert len(one.splitlines()) == nf
    assert run([exe, "r1w2", "05", str(first), "--rectify", cc, "--gpus", "2", "--same-device"], "r1w2") == one
    assert run([exe, "r1c3", "05", str(first), "--rectify", cc, "--gpus", "2", "--same-device", "--chunk", "3"], "r1c3") == one
    for w in (1, 2):
        got = run([sys.executable, "-m", "libviso_amd.kitti_shard", f"rd{w}", "05", str(first), "--gpus", str(w),
                   "--backend", "gloo", "--same-device", "--rectify", cc], f"rd{w}")
        assert got == one, w
    r = subprocess.run([exe, "nocalib", "05", str(first)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode != 0                                     # without --rectify it needs calib.txt

    # the batch API on the same raw frames: maps from the parsed file, Harris 1200 / 24 x 5, RANSAC keyed by the frame index
    cal = kitti_shard.load_cam_to_cam(cc)
    maps = [libviso_amd.rectify_map(cal["K"][s], cal["D"][s], cal["R"][s], cal["P"][s], cal["out_shape"]) for s in (0, 1)]
    P1, P2 = cal["P"]
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, nf, 1200)
    b.set_rectify(cal["raw_shape"], cal["out_shape"], left=maps[0], right=maps[1])
    b.upload_images_only(d["images"])
    b.detect(n_features=1200, nbinx=24, nbiny=5)
    param = Param.default(base=abs(P2[0, 3] / P2[0, 0]), f=P1[0, 0], cu=P1[0, 2], cv=P1[1, 2])
    b.set_params(MatchParams.stereo(libviso_amd.F_from_P(P1, P2)), MatchParams.temporal(), param, seed=0, first_frame=first)
    b.run_images()
    tr, ok, _ = b.poses()
    b.close(); ctx.close()
    poses, _ = hostmath.chain_poses(tr, ok)
    got = np.loadtxt(np.frombuffer(one, np.uint8).tobytes().decode().splitlines()).reshape(-1, 12)
    assert got.shape[0] == len(poses) and ok[1:].sum() >= nf - 2
    for g, p in zip(got, poses):
        assert np.abs(g - p[:3].reshape(-1)).max() < 2e-6 + 1e-5 * np.abs(p).max()
