"""The matcher kernels ON their fixed capacities: union list (448 entries per round), SAD8 store (176 rows), staged window
(512 keypoints + a tail in steps of 32), the pipeline's prologue / steady state / epilogue, the K cap, the overflow kernel's
staging area, the stereo kernel's chunks and slots, the batch kernel's pair-list segment.  The inputs are hand built
(tests/matcher_cases.py) and proven to sit where they claim without a device (tests/test_matcher_cases_cpu.py); here every
matcher variant of the build gives the oracle's matches on them, a batch gives the oracle's matches and scored-pair counter,
and match_union8_kernel hands over exactly the queries the case derives — an equality, never read from the device first."""
import numpy as np
import pytest

import libviso_amd
import matcher_cases as MC
from libviso_amd.abi import MatchParams, Param

pytestmark = pytest.mark.gpu

V8 = 6


def _direct(oracle, cases, variants):
    """libviso_amd.match_desc against the oracle for every case and variant (the planes' shift fixed at the families' 3)."""
    try:
        libviso_amd.set_row8_shift(MC.R8_SHIFT)
        want = [oracle.match_desc(*c.args()) for c in cases]
        assert all(len(w) >= 1 for w in want)
        for v in variants:
            libviso_amd.set_matcher_variant(v)
            for c, w in zip(cases, want):
                got = libviso_amd.match_desc(*c.args())
                assert np.array_equal(got, w), (c.name, v, len(got), len(w))
    finally:
        libviso_amd.set_matcher_variant(libviso_amd.DEFAULT_MATCHER)
        libviso_amd.set_row8_shift(-1)


def _batch(oracle, cases, stereo=False, derived=False):
    """The build's default variant through a Batch.  Temporal: the case in the left images of frames 0 (targets) and 1
    (queries), the right images empty.  Stereo: left (queries) and right (targets) of frame 0, frame 1 empty."""
    F = MC.rectified_F()
    ctx = libviso_amd.Context(0)
    try:
        libviso_amd.set_row8_shift(MC.R8_SHIFT, ctx)
        union8 = libviso_amd.DEFAULT_MATCHER == V8
        for c in cases:
            kp1, kp2, d1, d2, mp = c.args()
            n1, n2 = len(kp1), len(kp2)
            cap = max(n1, n2)
            kp = np.zeros((2, 2, cap, 2), np.float32)
            desc = np.zeros((2, 2, cap, MC.DLEN), np.float32)
            n = np.zeros((2, 2), np.int32)
            if stereo:
                kp[0, 0, :n1], desc[0, 0, :n1], kp[0, 1, :n2], desc[0, 1, :n2] = kp1, d1, kp2, d2
                n[0] = n1, n2
                which, t, st, tm = 0, 0, mp, MatchParams.temporal()
            else:
                kp[0, 0, :n2], desc[0, 0, :n2], kp[1, 0, :n1], desc[1, 0, :n1] = kp2, d2, kp1, d1
                n[0, 0], n[1, 0] = n2, n1
                which, t, st, tm = 1, 1, MatchParams.stereo(F), mp
            b = libviso_amd.Batch(ctx, 2, cap)
            try:
                b.upload(kp, desc, n)
                b.set_params(st, tm, Param.default(), seed=1)
                b.run_matcher()
                want, wsc = oracle.match_desc(kp1, kp2, d1, d2, mp, return_scored=True)
                got, sc, novf = b.matches(which, t), int(b.counters()[0][which, t]), b.overflow_count()
                assert np.array_equal(got, want) and sc == wsc, (c.name, len(got), len(want), sc, wsc)
                assert b.row8_shift() == MC.R8_SHIFT or not union8
                # the one other problem of the launch with queries (this frame's left image against an empty right image, or an
                # empty image against this one) has no candidate and hands nothing over: the count is this problem's
                if derived and union8:
                    assert novf == c.claims["ovf"], (c.name, novf, c.claims["ovf"], c.claims["nu"], c.claims["c"])
            finally:
                b.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("group", sorted(MC.TEMPORAL_GROUPS))
def test_direct_calls_every_variant(viso, oracle, group):
    _direct(oracle, MC.TEMPORAL_GROUPS[group](), libviso_amd.MATCHER_VARIANTS)


@pytest.mark.parametrize("group", sorted(MC.TEMPORAL_GROUPS))
def test_batch_results_counters_and_handed_over_queries(viso, oracle, group):
    """overflow_count is derived for the union list, store, pipeline, window and K-cap groups (both families; union8 only).
    For the overflow kernel's staging area and the batch kernel's segment every query of interest leaves the tile kernel by
    construction (or the count belongs to a kernel that is not the default): results and the scored counter only."""
    _batch(oracle, MC.TEMPORAL_GROUPS[group](), derived=group in MC.OVF_DERIVED)


def test_stereo_direct_call(viso, oracle):
    """The variant does not change the stereo kernel: once.  No derived hand-over count: a query leaves match_stereo_kernel for
    reasons of its own (more than K in radius), results and the scored counter decide."""
    _direct(oracle, MC.stereo_cases(), (libviso_amd.DEFAULT_MATCHER,))


def test_stereo_batch(viso, oracle):
    _batch(oracle, MC.stereo_cases(), stereo=True)
