"""The opt-in sub-pixel stereo refinement on the device (include/viso_hip.h, viso_batch_set_subpixel;
libviso_amd/csrc/subpixel.hip) against its numpy restatement (tests/subpixel_ref.py) and the CPU-assembled pipeline."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MatchParams

import subpixel_ref as S

pytestmark = pytest.mark.gpu


def _random_case(rng, rows, cols, n1, n2, n):
    imgL = rng.integers(0, 256, (rows, cols), dtype=np.uint8) if rng.random() < 0.5 else synth.make_images(int(rng.integers(1 << 30)), rows, cols)
    imgR = rng.integers(0, 256, (rows, cols), dtype=np.uint8) if rng.random() < 0.5 else synth.make_images(int(rng.integers(1 << 30)), rows, cols)
    kp1 = np.stack([rng.integers(0, cols, n1), rng.integers(0, rows, n1)], 1).astype(np.float32)
    kp2 = np.stack([rng.integers(0, cols, n2), rng.integers(0, rows, n2)], 1).astype(np.float32)
    kp1[: n1 // 4] += rng.uniform(-0.6, 0.6, (n1 // 4, 2)).astype(np.float32)    # non-integer keypoints round half to even
    match = np.stack([rng.integers(0, n1, n), rng.integers(0, n2, n), rng.integers(0, 9999, n)], 1).astype(np.int32)
    return imgL, imgR, kp1, kp2, match


def test_refine_equals_restatement(viso, oracle):
    rng = np.random.default_rng(11)
    for rows, cols in ((37, 53), (120, 301), (9, 9), (200, 640)):
        for rep in range(2):
            imgL, imgR, kp1, kp2, match = _random_case(rng, rows, cols, 300, 260, 500)
            # the image's edges: keypoints at 0, 1, cols-2, cols-1 and the same rows
            xs, ys = [0, 1, cols - 2, cols - 1], [0, 1, rows - 2, rows - 1]
            edge = np.array([[x, y] for x in xs for y in ys], np.float32)
            kp1[:16], kp2[:16] = edge, edge[::-1]
            match[:16, 0], match[:16, 1] = np.arange(16), np.arange(16)
            match[16:40, 1] = 7                                    # one right keypoint matched by many left ones
            for mode in (1, 2):
                got = libviso_amd.refine_stereo_subpixel(imgL, imgR, kp1, kp2, match, mode)
                want = S.refine(oracle, imgL, imgR, kp1, kp2, match, mode)
                assert got.dtype == np.float32 and np.array_equal(got, want), (rows, cols, mode)
    with pytest.raises(libviso_amd.VisoError):
        libviso_amd.refine_stereo_subpixel(imgL, imgR, kp1, kp2, match, 0)
    bad = match.copy(); bad[3, 1] = len(kp2)
    with pytest.raises(libviso_amd.VisoError):
        libviso_amd.refine_stereo_subpixel(imgL, imgR, kp1, kp2, bad, 1)


def _run(ctx, seq, mode, detect, seed=5, matcher_only=False, set_mode=True):
    nf = seq["kp"].shape[0]
    cap = seq["kp"].shape[2]
    b = libviso_amd.Batch(ctx, nf, cap)
    if detect:
        b.upload_images_only(seq["images"])
        b.detect(n_features=cap, nbinx=8, nbiny=3)
    else:
        b.upload_images(seq["images"], seq["kp"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=seed)
    if set_mode:
        b.set_subpixel(mode)
    b.run_images(matcher_only=matcher_only)
    return b


def _device_keypoints(b, seq):
    nf, _, cap, _ = seq["kp"].shape
    kp = np.zeros_like(seq["kp"]); n = np.zeros_like(seq["n"])
    for t in range(nf):
        for side in range(2):
            k = b.keypoints(t, side)
            kp[t, side, :len(k)] = k; n[t, side] = len(k)
    return dict(seq, kp=kp, n=n)


@pytest.fixture(scope="module")
def seq32():
    return synth.make_subpixel_image_sequence(8, 32, n_kp=600, width=640, height=200)


@pytest.mark.parametrize("detect", [False, True])
def test_batch_modes_against_cpu_pipeline(viso, oracle, seq32, detect):
    nf = seq32["kp"].shape[0]
    ctx = libviso_amd.Context(0)
    b0 = _run(ctx, seq32, 0, detect)
    seq = _device_keypoints(b0, seq32) if detect else seq32
    tr0, ok0, ni0 = b0.poses()
    for mode in (1, 2):
        b = _run(ctx, seq32, mode, detect)
        want = S.pipeline(oracle, seq, mode, seed=5)
        tr, ok, n_inl = b.poses()
        for t in range(nf):
            for which in range(3):
                if which and not t:
                    continue
                assert np.array_equal(b.matches(which, t), b0.matches(which, t)), (mode, which, t)
            assert np.array_equal(b.matches(0, t), want["lr"][t])
            uv = b.subpixel(t)
            assert np.array_equal(uv, want["uv"][t]), (mode, t)
        assert np.array_equal(ok, want["ok"]) and np.array_equal(n_inl, want["n_inl"]), mode
        assert detect or ok[1:].all()
        for t in range(1, nf):
            a, r = libviso_amd.tr2mat(tr[t]), oracle.tr2mat(want["tr"][t])
            assert np.linalg.norm(a - r) / np.linalg.norm(r) < 1e-5
        assert not np.array_equal(tr, tr0)
        # matcher_only: the refined points are produced all the same
        b.run_images(matcher_only=True)
        for t in (0, nf // 2, nf - 1):
            assert np.array_equal(b.subpixel(t), want["uv"][t])
        b.close()
    b0.close(); ctx.close()


def test_mode0_after_mode1_is_untouched(viso, seq32):
    ctx = libviso_amd.Context(0)
    ref = _run(ctx, seq32, 0, False, set_mode=False)
    b = _run(ctx, seq32, 1, False)
    b.set_subpixel(0)
    b.run_images()
    for got, want in zip(b.poses(), ref.poses()):
        assert np.array_equal(got, want)
    nf = seq32["kp"].shape[0]
    for t in range(nf):
        for which in range(3 if t else 1):
            assert np.array_equal(b.matches(which, t), ref.matches(which, t))
        c1, c2 = b.circle(t), ref.circle(t)
        assert np.array_equal(c1[0], c2[0]) and np.array_equal(c1[1], c2[1])
    with pytest.raises(libviso_amd.VisoError):   # the last run refined nothing
        b.subpixel(1)
    b.close(); ref.close(); ctx.close()


def test_descriptor_in_run_refuses_a_mode(viso, oracle):
    seq = synth.make_sequence(4, 4, n_kp=400, width=500, height=200)
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 4, 400)
    b.upload(seq["kp"], seq["desc"], seq["n"])
    b.set_params(st, tm, seq["param"], seed=1)
    for mode in (1, 2):
        b.set_subpixel(mode)
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b.run()
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b.run_matcher()
    with pytest.raises(libviso_amd.VisoError):
        b.set_subpixel(3)
    b.set_subpixel(0)
    b.run()
    tr, ok, n_inl = b.poses()
    want = oracle.sequence(seq["kp"], seq["desc"], seq["n"], st, tm, seq["param"], seed=1)
    assert np.array_equal(ok, want["ok"]) and np.array_equal(n_inl, want["n_inl"])
    b.close(); ctx.close()


def test_refinement_lowers_the_device_translation_error(viso):
    # the scene and margin of tests/test_subpixel_cpu.py (measured there on the CPU assembly: median 6.1 -> 5.2 mm)
    seq = synth.make_subpixel_image_sequence(2, 24, n_kp=1500)
    ctx = libviso_amd.Context(0)
    err = {}
    for mode in (0, 1):
        b = _run(ctx, seq, mode, False, seed=3)
        tr, ok, _ = b.poses()
        assert ok[1:].all()
        err[mode] = np.median(S.translation_errors(tr, seq["tr_gt"]))
        b.close()
    ctx.close()
    assert err[1] < 0.95 * err[0], err


def test_kitti_runners_with_subpixel_write_one_pose_file(tmp_path):
    """viso_kitti / kitti_shard --subpixel 1: a chunk's halo frame is refined again like any other frame, so every partition
    (and chunking) writes the byte-identical pose file, and it differs from the one without refinement."""
    import os
    import subprocess
    import sys

    import kitti_tree
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    assert os.path.exists(exe), "libviso_amd/viso_kitti is missing: run __graft_entry__.build()"
    home, first, nf = str(tmp_path), 3, 11
    seq = synth.make_subpixel_image_sequence(21, nf, n_kp=1500, width=720, height=240)
    kitti_tree.write_tree(home, "04", seq, first_index=first)
    env = dict(os.environ, KITTI_HOME=home, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(cmd, sha):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert r.returncode == 0, r.stdout + r.stderr
        return open(os.path.join(home, "results", "04", sha, "data", "04.txt"), "rb").read()

    off = run([exe, "sp0", "04", str(first), "--subpixel", "0"], "sp0")
    one = run([exe, "sp1", "04", str(first), "--subpixel", "1"], "sp1")
    assert len(one.splitlines()) == nf and one != off
    assert run([exe, "sp1w2", "04", str(first), "--subpixel", "1", "--gpus", "2", "--same-device"], "sp1w2") == one
    assert run([exe, "sp1c3", "04", str(first), "--subpixel", "1", "--gpus", "2", "--same-device", "--chunk", "3"], "sp1c3") == one
    for w in (1, 2):
        got = run([sys.executable, "-m", "libviso_amd.kitti_shard", f"spd{w}", "04", str(first), "--gpus", str(w),
                   "--backend", "gloo", "--same-device", "--subpixel", "1"], f"spd{w}")
        assert got == one, w
    r = subprocess.run([exe, "bad", "04", str(first), "--subpixel", "3"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode != 0
