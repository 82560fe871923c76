"""sort_matches_kernel and sort_kp_kernel at the sizes where their code takes another path, through the batch C-ABI.

sort_matches: temporal problems whose accepted set and SADs are chosen here -- every query sits alone on a coarse grid,
an accepted query has exactly one target in radius (its twin, whose descriptor differs in one element by the distance
wanted), a rejected one has none -- so the expected list is known without the device: the accepted (i1, i2, dist) rows in
numpy.lexsort((i1, dist)) order.  The count (m_cnt) is the list's length; pos (the list's inverse permutation) is what the
circle join walks, so the circle is compared with the oracle's join of the very lists the batch returned.  Capacities 2048
and 2049 sit on either side of a doubling of the kernel's key arrays (padded to a power of two).

sort_kp: image sizes around a wave, the workgroup and what a thread keeps in registers (2048 per image), NaN x, all x
equal; its outputs (bucket order, bstart, rank, qord) have no getter in the C-ABI, they are checked by what every matcher
kernel makes of them: all lists of both frames equal to the oracle's."""
import numpy as np
import pytest

import libviso_amd
import matcher_cases as MC
from libviso_amd import synth
from libviso_amd.abi import MatchParams, Param

pytestmark = pytest.mark.gpu

DLEN = 121
N1 = 2000          # queries of every sort_matches case
STEP = 1000.0      # grid pitch: far beyond the radius (80), a query sees its twin only


def _grid(idx):
    idx = np.asarray(idx)
    return np.stack([STEP * (idx % 50), STEP * (idx // 50)], 1).astype(np.float32)


def _sort_case(rng, m, dists):
    """(kp1, d1, kp2, d2, want): N1 queries, m of them (a random subset) accepted with the SADs `dists` (one per accepted
    query, in the subset's order); want = the sorted rows."""
    acc = np.sort(rng.choice(N1, m, replace=False))
    kp1 = _grid(np.arange(N1))
    d1 = rng.integers(-100, 101, (N1, DLEN)).astype(np.float32)
    order = rng.permutation(m)                       # target 1 + j is the twin of query acc[order[j]]
    kp2 = np.concatenate([np.array([[-5000.0, -5000.0]], np.float32), kp1[acc[order]]])   # target 0: out of every radius (Q1)
    d2 = np.concatenate([np.zeros((1, DLEN), np.float32), d1[acc[order]]])
    dists = np.asarray(dists, np.int64)
    d2[1:, 7] += dists[order].astype(np.float32)
    i2 = np.empty(m, np.int64)
    i2[order] = 1 + np.arange(m)
    rows = np.stack([acc, i2, dists], 1).astype(np.int32)
    want = rows[np.lexsort((rows[:, 0], rows[:, 2]))] if m else rows.reshape(0, 3)
    return kp1, d1, kp2, d2, want


def _run_sort_case(oracle, cap, kp1, d1, kp2, d2, want):
    n1, n2 = len(kp1), len(kp2)
    kp = np.zeros((2, 2, cap, 2), np.float32)
    desc = np.zeros((2, 2, cap, DLEN), np.float32)
    n = np.zeros((2, 2), np.int32)
    for side in range(2):                            # the right images are the left ones: the stereo lists (all SADs 0) feed the circle
        kp[0, side, :n2], desc[0, side, :n2], kp[1, side, :n1], desc[1, side, :n1] = kp2, d2, kp1, d1
    n[0], n[1] = n2, n1
    st, tm = MatchParams.stereo(MC.rectified_F()), MatchParams.temporal()
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 2, cap)
    try:
        b.upload(kp, desc, n)
        b.set_params(st, tm, Param.default(), seed=1)
        b.run()
        for which in (1, 2):
            got = b.matches(which, 1)
            assert len(got) == len(want), (which, len(got), len(want))                  # m_cnt
            assert np.array_equal(got, want), (which, np.flatnonzero((got != want).any(1))[:5])
        assert np.array_equal(want, oracle.match_desc(kp1, kp2, d1, d2, tm))           # (the construction itself)
        lr, lrp = b.matches(0, 1), b.matches(0, 0)
        assert np.array_equal(lr, oracle.match_desc(kp1, kp1, d1, d1, st))
        assert np.array_equal(lrp, oracle.match_desc(kp2, kp2, d2, d2, st))
        circ, pcl = b.circle(1)                                                          # pos of all four lists
        _, wc, wp, _ = oracle.match_circle(lr, lrp, b.matches(1, 1), b.matches(2, 1))
        assert np.array_equal(circ, wc) and np.array_equal(pcl, wp)
        return len(circ)
    finally:
        b.close(); ctx.close()


@pytest.mark.parametrize("m", [0, 1, 2, 64, 65, 1999, 2000])
def test_sort_matches_counts(viso, oracle, m):
    """Random SADs in 0..5000 (ties among them: the i1 order decides), 0 to N1 accepted of N1 queries."""
    rng = np.random.default_rng(100 + m)
    case = _sort_case(rng, m, rng.integers(0, 5001, m))
    n_circ = _run_sort_case(oracle, 2048, *case)
    assert n_circ > 0 or m < 64


@pytest.mark.parametrize("cap", [2048, 2049])
@pytest.mark.parametrize("kind", ["random", "equal", "outlier"])
def test_sort_matches_distributions(viso, oracle, cap, kind):
    """equal: every SAD the same -- one bucket holds all 1500 keys, more than VISO_SORT_BMAX: the bitonic network.  outlier:
    a narrow peak and one SAD of 30000 -- the peak keeps the fine buckets, the outlier lands in the log-linear tail."""
    rng = np.random.default_rng(7)
    m = 2000 if kind == "random" else 1500
    dists = {"random": rng.integers(0, 5001, m), "equal": np.full(m, 77), "outlier": rng.integers(100, 201, m)}[kind]
    if kind == "outlier":
        dists[m // 2] = 30000
    _run_sort_case(oracle, cap, *_sort_case(rng, m, dists))


@pytest.fixture(scope="module")
def kp_seq():
    return synth.make_sequence(77, 2, n_kp=2049, width=1241, height=376)


def _run_kp_case(oracle, seq, nk, edit=None):
    cap = max(nk, 1)
    kp = np.ascontiguousarray(seq["kp"][:, :, :cap]).copy()
    desc = np.ascontiguousarray(seq["desc"][:, :, :cap])
    n = np.full((2, 2), nk, np.int32)
    if edit:
        edit(kp)
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 2, cap)
    try:
        b.upload(kp, desc, n)
        b.set_params(st, tm, seq["param"], seed=1)
        b.run_matcher()
        total = 0
        for which, t in ((0, 0), (0, 1), (1, 1), (2, 1)):
            q = (0, t) if which < 2 else (1, t)
            g = (1, t) if which == 0 else ((0, t - 1) if which == 1 else (1, t - 1))
            want = oracle.match_desc(kp[q[1], q[0], :nk], kp[g[1], g[0], :nk], desc[q[1], q[0], :nk], desc[g[1], g[0], :nk],
                                     st if which == 0 else tm)
            got = b.matches(which, t)
            assert np.array_equal(got, want), (nk, which, t, len(got), len(want))
            total += len(got)
        return total
    finally:
        b.close(); ctx.close()


@pytest.mark.parametrize("nk", [0, 1, 63, 64, 65, 255, 256, 257, 2000, 2049])
def test_sort_kp_image_sizes(viso, oracle, kp_seq, nk):
    total = _run_kp_case(oracle, kp_seq, nk)
    assert total > 0 or nk < 255, (nk, total)


def test_sort_kp_nan_x(viso, oracle, kp_seq):
    """NaN x: the last bucket, out of every radius."""
    def edit(kp):
        kp[:, :, 5:300:7, 0] = np.nan
    assert _run_kp_case(oracle, kp_seq, 300, edit) > 50


def test_sort_kp_all_x_equal(viso, oracle, kp_seq):
    """One column: the bucket map's scale is 0, every keypoint in bucket 0, every window the whole image."""
    def edit(kp):
        kp[..., 0] = 100.0
    _run_kp_case(oracle, kp_seq, 300, edit)
