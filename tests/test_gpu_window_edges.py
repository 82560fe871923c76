"""The sliding-window bundle adjustment on the device (libviso_amd/csrc/window.hip) where its definition has edges: forks, breaks,
duplicate entries, extreme keys, empty frames, the failure statuses and the edges of the kernel's track chunks through the direct
call, and a batch with planted forks and breaks (K = 2..5, chunking with breaks in the halo, changing K on one batch, small
batches, the K = 2 identity, the motion refinement and covariance on the same frames), and full-size windows; every record is
compared with the numpy restatement (tests/window_ref.py) by tests/window_cases.check."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth

import window_ref as WR
from estimator_util import seq_batch
from test_gpu_covariance import _check_batch_frames as covariance_batch_frames
from test_gpu_refine import _check_batch_frames as refine_batch_frames
from window_cases import (HAND_CASES, check, check_k2_identity, chunk_case, chunk_sizes, direct_frames, hand_case,
                          wn_chunk)

pytestmark = pytest.mark.gpu

MODES = ((1, None), (2, 0.3))
PLANTED = (9, 21, 33)          # frames cut to two keypoints per image: each is a break, and so is the frame after it


def _direct_against_restatement(frames, param, expected, what):
    length = len(frames)
    for mode, sigma in MODES:
        with np.errstate(all="ignore"):
            want = WR.window(frames, length - 1, length, param, mode, sigma)
        assert (want["status"], want["len"], want["n_points"]) == expected, (what, mode)
        got = libviso_amd.window_refine(direct_frames(frames), param, mode=mode, sigma=sigma)
        check(got, want, (what, mode))     # status, len, n_points, n_rows exact; tr, tr_win byte-equal when status != 1


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_built_windows(viso, name):
    frames, param, expected = hand_case(name)
    _direct_against_restatement(frames, param, expected, name)


def test_a_list_longer_than_its_frame_is_refused(viso):
    # the direct call takes n_inl <= m (include/viso_hip.h): a list with an index twice is refused when it is longer than m
    frames, param, _want = hand_case("row_twice")
    frs = direct_frames(frames)
    X, obs, left, tr, inl = frs[1]
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        libviso_amd.window_refine([frs[0], (X, obs, left, tr, np.arange(X.shape[1] + 1) % X.shape[1]), frs[2]], param)


@pytest.mark.parametrize("length", [2, 3, 4, 5])
def test_windows_at_the_chunk_edges(viso, length):
    # 6 (the fewest tracks a formed window has), CH - 1, CH, CH + 1 (a last chunk of one track) and 2 CH tracks
    for n in chunk_sizes(length):
        frames, param, expected = chunk_case(length, n)
        _direct_against_restatement(frames, param, expected, (length, n, wn_chunk(length)))


@pytest.fixture(scope="module")
def planted():
    seq = synth.make_noisy_sequence(31, 48, 0.3, n_kp=1200, dup_frac=0.1, ragged=True)
    for t in PLANTED:
        seq["n"][t] = [2, 2]
    return seq


def _breaks_planted(b):
    ok = b.poses()[1]
    for t in PLANTED:
        assert ok[t] == 0 and ok[t + 1] == 0, t


@pytest.mark.parametrize("K", [2, 3, 4, 5])
def test_batch_with_planted_forks_and_breaks(viso, planted, K):
    ctx = libviso_amd.Context(0)
    b = seq_batch(ctx, planted, window=(K,))
    _breaks_planted(b)
    recs = b.window_refines()
    frames = WR.frames_from_batch(b)
    forks = sum(int(v == -2) for fr in frames[1:] for tab in WR.tables(fr) for v in tab.values())
    moved = n_valid = 0
    for t in range(b.nf):
        want = WR.window(frames, t, K, planted["param"], 1)
        check(recs[t], want, (K, t))
        n_valid += want["status"] == 1
        moved += want["status"] == 1 and want["len"] < min(K, t + 1)
    for t in PLANTED:
        assert int(recs[t]["status"]) == 0 and int(recs[t + 1]["status"]) == 0, t
    print(f"\nK={K}: {forks} fork keys in the L' tables, {moved} windows cut short by a break, {n_valid} valid")
    assert forks >= 5                           # the data reached the fork paths ...
    if K >= 3:
        assert moved >= len(PLANTED)            # ... and the break rule moved anchors
    assert n_valid >= 35
    b.close(); ctx.close()


def test_chunks_with_breaks_in_the_halo(viso, planted):
    K = 4
    ctx = libviso_amd.Context(0)
    b = seq_batch(ctx, planted, window=(K,))
    whole = b.window_refines()
    b.close()
    # chunk 2's halo (frames 20, 21, 22) holds the breaks 21 and 22; chunk 3's halo begins at the planted frame 33
    bounds = (0, 23, 36, 48)
    for c0, c1 in zip(bounds[:-1], bounds[1:]):
        first = max(c0 - (K - 1), 0)
        bc = seq_batch(ctx, planted, window=(K,), first=first, frames=slice(first, c1))
        got = bc.window_refines()
        h = max(c0 - first, 1)
        assert got[h:].tobytes() == whole[first + h:c1].tobytes(), (c0, c1)
        bc.close()
    for t in (21, 22, 33, 34):
        assert int(whole["status"][t]) == 0, t
    ctx.close()


def test_changing_K_on_one_batch(viso, planted):
    ctx = libviso_amd.Context(0)
    b = seq_batch(ctx, planted, window=(5,))
    r5 = b.window_refines()
    b.set_window_refine(3)                      # a smaller K in the buffers allocated for 5
    b.run()
    r3 = b.window_refines()
    fresh = seq_batch(ctx, planted, window=(3,))
    assert r3.tobytes() == fresh.window_refines().tobytes()
    fresh.close()
    b.set_window_refine(5)                      # back, without reallocating
    b.run()
    assert b.window_refines().tobytes() == r5.tobytes()
    assert r3["len"].max() == 3 and r5["len"].max() == 5
    b.close()
    b2 = seq_batch(ctx, planted, window=(2,))
    b2.set_window_refine(4)                     # a larger K: reallocated, zeroed buffers
    b2.run()
    fresh = seq_batch(ctx, planted, window=(4,))
    assert b2.window_refines().tobytes() == fresh.window_refines().tobytes()
    b2.close(); fresh.close(); ctx.close()


def test_small_batches(viso, planted):
    ctx = libviso_amd.Context(0)
    for first, nf in ((0, 2), (0, 3), (11, 3), (34, 2)):
        b = seq_batch(ctx, planted, window=(5,), first=first, frames=slice(first, first + nf))
        recs = b.window_refines()
        frames = WR.frames_from_batch(b)
        for t in range(nf):
            check(recs[t], WR.window(frames, t, 5, planted["param"], 1), (first, nf, t))
        assert recs["len"].max() <= nf
        b.close()
    ctx.close()


def test_k2_identity_with_breaks(viso, planted):
    ctx = libviso_amd.Context(0)
    b = seq_batch(ctx, planted, refine=(1,), window=(2,))
    w, r = b.window_refines(), b.refines()
    assert check_k2_identity(w, r) >= 35
    for t in PLANTED:
        assert int(w[t]["status"]) == int(r[t]["status"]) == 0 and int(w[t + 1]["status"]) == int(r[t + 1]["status"]) == 0
    b.close(); ctx.close()


def test_motion_refinement_and_covariance_with_breaks(viso, planted):
    ctx = libviso_amd.Context(0)
    for mode, sigma in ((1, None), (2, 0.3)):
        b = seq_batch(ctx, planted, cov=(mode, sigma), refine=(mode, sigma))
        _breaks_planted(b)
        assert refine_batch_frames(b, planted["param"], mode, sigma) >= 35
        assert covariance_batch_frames(b, planted["param"], mode, sigma) >= 35
        for t in PLANTED:
            for recs in (b.refines(), b.covariances()):
                assert int(recs[t]["status"]) == 0 and int(recs[t + 1]["status"]) == 0, t
        b.close()
    ctx.close()


def test_full_size_windows(viso):
    seq = synth.make_noisy_sequence(41, 12, 0.3, n_kp=2000)
    K = 5
    ctx = libviso_amd.Context(0)
    b = seq_batch(ctx, seq, window=(K,))
    recs = b.window_refines()
    frames = WR.frames_from_batch(b)
    off_edge = {}
    for t in range(b.nf):
        want = WR.window(frames, t, K, seq["param"], 1)
        check(recs[t], want, t)
        if want["status"] == 1:
            off_edge.setdefault(want["len"], []).append(want["n_points"] % wn_chunk(want["len"]) != 0)
    print(f"\nwindows per len: { {k: len(v) for k, v in sorted(off_edge.items())} }, most tracks {recs['n_points'].max()}")
    assert max(off_edge) == K and recs["n_points"].max() >= 1200
    for length, flags in off_edge.items():
        assert any(flags), length               # a last chunk that is only partly full, at every len that occurs
    b.close(); ctx.close()
