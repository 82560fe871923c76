"""The opt-in sliding-window bundle adjustment on the device (include/viso_hip.h, "window refinement"; libviso_amd/csrc/window.hip)
against its numpy restatement (tests/window_ref.py): the batch for K = 2..5, the K = 2 identity with the motion refinement, the
direct call, chunking with a K - 1 halo, invariance of everything else, getter errors, the image-in path, and accuracy on a noisy
synthetic sequence."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MatchParams

import window_ref as WR
from estimator_util import seq_batch
from window_cases import check, check_k2_identity

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def noisy40():
    return synth.make_noisy_sequence(23, 40, 0.3, n_kp=1200)


@pytest.mark.parametrize("K", [2, 3, 4, 5])
def test_batch_against_the_restatement(viso, noisy40, K):
    ctx = libviso_amd.Context(0)
    b = seq_batch(ctx, noisy40, window=(K,))
    recs = b.window_refines()
    frames = WR.frames_from_batch(b)
    n_valid, lens = 0, []
    for t in range(b.nf):
        want = WR.window(frames, t, K, noisy40["param"], 1)
        check(recs[t], want, (K, t))
        assert recs[t].tobytes() == b.window_refine(t).tobytes()
        n_valid += want["status"] == 1
        lens.append(want["len"])
    assert n_valid >= 35 and max(lens) == K
    b.close(); ctx.close()


def test_k2_records_agree_with_the_motion_refinement(viso, noisy40):
    ctx = libviso_amd.Context(0)
    b = seq_batch(ctx, noisy40, refine=(1,), window=(2,))
    assert check_k2_identity(b.window_refines(), b.refines()) >= 35
    b.close(); ctx.close()


@pytest.mark.parametrize("K", [3, 5])
def test_direct_call_is_byte_identical_to_the_batch(viso, noisy40, K):
    ctx = libviso_amd.Context(0)
    b = seq_batch(ctx, noisy40, window=(K, 2, 0.3))
    recs = b.window_refines()
    n = 0
    for t in range(1, b.nf):
        L = int(recs[t]["len"])
        if int(recs[t]["status"]) != 1:
            continue
        frames = []
        for j in range(t - L + 2, t + 1):
            X, obs = b.points(j)
            circ, _ = b.circle(j)
            _ok, tr, inl = b.pose(j)
            frames.append((X, obs, circ[:, [0, 2]], tr, inl))
        got = libviso_amd.window_refine(frames, noisy40["param"], mode=2, sigma=0.3)
        assert got.tobytes() == recs[t].tobytes(), t
        n += 1
    assert n >= 30
    b.close(); ctx.close()


def test_chunked_batches_give_byte_equal_records(viso, noisy40):
    K = 4
    ctx = libviso_amd.Context(0)
    whole = seq_batch(ctx, noisy40, window=(K,)).window_refines()
    c0 = 20
    ba = seq_batch(ctx, noisy40, window=(K,), frames=slice(0, c0))
    bc = seq_batch(ctx, noisy40, window=(K,), first=c0 - (K - 1), frames=slice(c0 - (K - 1), 40))   # a K - 1 frame halo
    a, c = ba.window_refines(), bc.window_refines()
    assert a[1:].tobytes() == whole[1:c0].tobytes()
    assert c[K - 1:].tobytes() == whole[c0:].tobytes()
    assert (whole["status"][1:] == 1).sum() >= 35
    ctx.close()


def test_window_on_and_off_leave_everything_else_identical(viso, noisy40):
    ctx = libviso_amd.Context(0)
    b0 = seq_batch(ctx, noisy40, cov=(1,), refine=(1,))
    b1 = seq_batch(ctx, noisy40, cov=(1,), refine=(1,), window=(5,))
    for x, y in zip(b0.poses(), b1.poses()):
        assert x.tobytes() == y.tobytes()
    for t in range(b0.nf):
        p0, p1 = b0.pose(t), b1.pose(t)
        assert p0[0] == p1[0] and p0[1].tobytes() == p1[1].tobytes() and p0[2].tobytes() == p1[2].tobytes()
    assert b0.covariances().tobytes() == b1.covariances().tobytes()
    assert b0.refines().tobytes() == b1.refines().tobytes()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b0.window_refines()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b0.window_refine(3)
    b1.set_window_refine(0)
    b1.run()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b1.window_refines()
    for K, mode, sigma in ((1, 1, None), (6, 1, None), (3, 3, None), (3, 2, -1.0), (3, 2, float("nan"))):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b1.set_window_refine(K, mode, sigma)
    b1.set_window_refine(3)
    b1.run()
    assert b1.window_refines()["status"][1:].max() == 1
    b0.close(); b1.close(); ctx.close()


def test_image_in_path_with_subpixel(viso):
    seq = synth.make_subpixel_image_sequence(8, 16, n_kp=600, width=640, height=200)
    ctx = libviso_amd.Context(0)
    nf, cap = seq["kp"].shape[0], seq["kp"].shape[2]
    b = libviso_amd.Batch(ctx, nf, cap)
    b.upload_images(seq["images"], seq["kp"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=5)
    b.set_subpixel(1)
    b.set_window_refine(3)
    b.run_images()
    recs = b.window_refines()
    frames = WR.frames_from_batch(b)
    n_valid = 0
    for t in range(nf):
        want = WR.window(frames, t, 3, seq["param"], 1)
        check(recs[t], want, t)
        n_valid += want["status"] == 1
    assert n_valid >= 10
    b.run_images(matcher_only=True)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.window_refines()
    b.run_images()                     # usable again
    assert b.window_refines()["status"][1:].max() == 1
    b.close(); ctx.close()


def test_accuracy_on_a_noisy_sequence(viso):
    sigma = 0.3
    seq = synth.make_noisy_sequence(17, 257, sigma)
    gt = seq["tr_gt"]
    ctx = libviso_amd.Context(0)
    b = seq_batch(ctx, seq, window=(2, 2, sigma))
    r2 = b.window_refines()
    b.set_window_refine(4, 2, sigma)
    b.run()
    r4 = b.window_refines()
    good = np.nonzero((r2["status"] == 1) & (r4["status"] == 1))[0]
    assert len(good) >= 250

    def med(recs, sl):
        return float(np.median(np.linalg.norm(recs["tr"][good][:, sl] - gt[good][:, sl], axis=1)))

    rot = (med(r2, slice(0, 3)), med(r4, slice(0, 3)))
    tra = (med(r2, slice(3, 6)), med(r4, slice(3, 6)))
    e4 = r4["tr"][good] - gt[good]
    nees = np.array([e @ np.linalg.solve(r4[t]["cov"], e) for t, e in zip(good, e4)])
    print(f"\nmedian rotation error K=2 {rot[0]:.3e} K=4 {rot[1]:.3e} (ratio {rot[1] / rot[0]:.3f}); translation "
          f"{tra[0]:.3e} -> {tra[1]:.3e} (ratio {tra[1] / tra[0]:.3f}); K=4 mean NEES {nees.mean():.3f}; "
          f"mean len {r4['len'][good].mean():.2f}")
    assert rot[1] < rot[0] and tra[1] < tra[0]
    # the CPU Monte Carlo (tests/test_window_cpu.py) measures 5.82 with the true sigma; the device band of the motion covariance
    # and refinement ([5.0, 7.2]) holds it and this sequence's 256 frames (standard error ~0.22)
    assert 5.0 <= float(nees.mean()) <= 7.2
    assert np.all(r4["gap"][good] < 1e-3)
    b.close(); ctx.close()
