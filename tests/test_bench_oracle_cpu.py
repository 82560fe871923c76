"""The chunked, threaded oracle of tests/bench_oracle.py is bit-equal to one whole oracle.sequence call: every
bench-sized GPU comparison (tests/test_gpu_bench_batch.py) rests on that."""
import numpy as np
import pytest

from libviso_amd import synth
from libviso_amd.abi import MatchParams

import bench_oracle


@pytest.fixture(scope="module")
def seq():
    return synth.make_sequence(108, 40, n_kp=300, width=400, height=160)


@pytest.mark.parametrize("first_frame", [0, 512])
@pytest.mark.parametrize("matcher_only", [False, True])
def test_chunked_sequence_equals_one_call(oracle, seq, first_frame, matcher_only):
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    whole = oracle.sequence(seq["kp"], seq["desc"], seq["n"], st, tm, seq["param"], seed=1, first_frame=first_frame,
                            matcher_only=matcher_only)
    if not matcher_only:
        assert whole["ok"][1:].sum() >= 30              # the poses compared are real ones
    assert whole["m_out"][1:, 1:].min() > 0
    for chunk, workers in ((2, 4), (3, 16), (7, 3), (16, 2), (40, 1), (64, 5)):
        got = bench_oracle.sequence_chunked(seq["kp"], seq["desc"], seq["n"], st, tm, seq["param"], seed=1,
                                            first_frame=first_frame, workers=workers, chunk=chunk,
                                            matcher_only=matcher_only)
        for key in ("tr", "ok", "n_inl", "scored", "m_out"):
            assert got[key].shape == whole[key].shape, (key, chunk)
            assert np.array_equal(got[key], whole[key]), (key, chunk, first_frame)
    # the default chunking too
    got = bench_oracle.sequence_chunked(seq["kp"], seq["desc"], seq["n"], st, tm, seq["param"], seed=1,
                                        first_frame=first_frame, matcher_only=matcher_only)
    assert all(np.array_equal(got[k], whole[k]) for k in ("tr", "ok", "n_inl", "scored", "m_out"))


def test_first_frame_changes_the_poses(oracle, seq):
    """The RANSAC key really is first_frame + t: a chunk that passed the wrong key would not go unnoticed above."""
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    a = bench_oracle.sequence_chunked(seq["kp"][:12], seq["desc"][:12], seq["n"][:12], st, tm, seq["param"], seed=1)
    b = bench_oracle.sequence_chunked(seq["kp"][:12], seq["desc"][:12], seq["n"][:12], st, tm, seq["param"], seed=1,
                                      first_frame=512)
    assert not np.array_equal(a["tr"], b["tr"])


def test_lists_equal_the_sequence_counters(oracle, seq):
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    whole = oracle.sequence(seq["kp"], seq["desc"], seq["n"], st, tm, seq["param"], seed=1, matcher_only=True)
    frames = [0, 1, 7, 8, 9, 39]
    got = bench_oracle.lists(seq, frames, (0, 1, 2), st, tm, workers=4)
    assert sorted(got) == sorted((w, t) for t in frames for w in range(3) if w == 0 or t >= 1)
    for (w, t), (m, sc) in got.items():
        assert len(m) == whole["m_out"][w, t] and sc == whole["scored"][w, t], (w, t)
        want = bench_oracle.match_one(seq, w, t, st, tm)
        assert np.array_equal(m, want[0]) and sc == want[1]
