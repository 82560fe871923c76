"""subpixel_refine_kernel (libviso_amd/csrc/subpixel.hip) at its staging borders, roundings, cost ties, list lengths and
degenerate images, bit for bit against the numpy restatement (tests/subpixel_ref.py): the direct call (left windows from the
image) and small hand-built batches (left windows from the packed u16 rows).  The cases and what each one reaches are in
tests/subpixel_cases.py; tests/test_subpixel_cases_cpu.py proves on the CPU that they reach it."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import hostmath, synth
from libviso_amd.abi import MatchParams, Param

import subpixel_cases as SC
import subpixel_ref as S

pytestmark = pytest.mark.gpu


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _first_difference(oracle, case, mode, got, want, what):
    """The report of a failure: the shape, the mode and the first differing row's q, staging path and cost classes."""
    imgL, imgR, kp1, kp2, match = case
    rows, cols = imgL.shape
    bad = np.flatnonzero((_bits(got) != _bits(want)).any(1))
    r = int(bad[0])
    q = SC.row_q(kp2, match[r:r + 1])[0]
    msg = "%s: %d x %d (cols & 3 = %d), mode %d, %d of %d rows differ; row %d: kp1 %s kp2 %s q %s is_fast %s got %s want %s" % (
        what, rows, cols, cols & 3, mode, len(bad), len(match), r, kp1[match[r, 0]].tolist(), kp2[match[r, 1]].tolist(),
        q.tolist(), bool(SC.is_fast(q, rows, cols)), got[r].tolist(), want[r].tolist())
    if max(np.abs(kp1[match[r, 0]]).max(), np.abs(kp2[match[r, 1]]).max()) <= SC.FAR_OK:   # the oracle is defined there
        Sx, Sy = S.costs(oracle, imgL, imgR, kp1, kp2, match[r:r + 1])
        msg += " Sx %s (%s) Sy %s (%s)" % (Sx[0].tolist(), SC.cost_class(*Sx[0]).item(), Sy[0].tolist(), SC.cost_class(*Sy[0]).item())
    return msg


def _check_direct(oracle, case, what, expect=None):
    """viso_refine_stereo_subpixel on the case in modes 1 and 2 == the expectation, as uint32 (so -0 is not +0)."""
    for mode in (1, 2):
        want = S.refine(oracle, *case, mode) if expect is None else expect(mode)
        got = libviso_amd.refine_stereo_subpixel(*case, mode)
        assert got.dtype == np.float32 and got.shape == want.shape, (what, mode, got.shape, want.shape)
        if not np.array_equal(_bits(got), _bits(want)):
            pytest.fail(_first_difference(oracle, case, mode, got, want, what))


# ------------------------------------------------------------------------------------------------------- direct call
@pytest.mark.parametrize("kind", ["random", "smooth"])
@pytest.mark.parametrize("shape", SC.EVERY_SHAPES, ids=_ids)
def test_every_position(viso, oracle, shape, kind):
    _check_direct(oracle, SC.every_position(*shape, kind), "every position, %s" % kind)


def test_rounding(viso, oracle):
    _check_direct(oracle, SC.rounding(), "rounding")


@pytest.mark.parametrize("which", ["right", "left", "both"])
def test_far_away_within_the_oracle(viso, oracle, which):
    _check_direct(oracle, SC.far_away(which, SC.FAR_SMALL), "far away (<= 2^20), %s" % which)


@pytest.mark.parametrize("which", ["right", "left", "both"])
def test_far_away_beyond_an_int(viso, oracle, which):
    """|coordinate| from 2^31 to 3e38: the expectation is the header's definition with the windows outside the image
    written down as zeros (SC.analytic_refine; equal to the restatement at 2^20, tests/test_subpixel_cases_cpu.py)."""
    case = SC.far_away(which, SC.FAR_HUGE)
    _check_direct(oracle, case, "far away (>= 2^31), %s" % which,
                  expect=lambda mode: SC.analytic_refine(oracle.extract_descriptors, *case, mode))


def test_ties(viso, oracle):
    for name, case, cx, cy in SC.ties(oracle):
        _check_direct(oracle, case, "ties, %s" % name)


@pytest.mark.parametrize("kind", SC.LENGTH_KINDS)
def test_list_lengths(viso, oracle, kind):
    for n in SC.LENGTHS:
        _check_direct(oracle, SC.list_length(n, kind), "list of %d rows, %s" % (n, kind))


@pytest.mark.parametrize("shape", SC.DEGENERATE_SHAPES, ids=_ids)
def test_degenerate_shapes(viso, oracle, shape):
    _check_direct(oracle, SC.degenerate(*shape), "degenerate")


# -------------------------------------------------------------------------------------------------------- batch path
def _check_batch(b, oracle, case, mode, what):
    """Every frame's stereo list == the oracle's, its refined points == the restatement on that list, bit for bit and of
    exactly that length.  Returns the device's lists."""
    lists = []
    for t, (m, uv) in enumerate(SC.batch_expected(oracle, case, mode)):
        got_m = b.matches(0, t).reshape(-1, 3)
        assert np.array_equal(got_m, m.reshape(-1, 3)), (what, mode, t, len(got_m), len(m))
        got = b.subpixel(t)
        assert got.dtype == np.float32 and got.shape == uv.shape, (what, mode, t, got.shape, uv.shape)
        if not np.array_equal(_bits(got), _bits(uv)):
            nL, nR = case["n"][t]
            frame = (case["images"][t, 0], case["images"][t, 1], case["kp"][t, 0, :nL], case["kp"][t, 1, :nR], m)
            pytest.fail(_first_difference(oracle, frame, mode, got, uv, "%s, frame %d" % (what, t)))
        lists.append(got_m)
    return lists


@pytest.mark.parametrize("small", [True, False], ids=["cap5", "lattice"])
@pytest.mark.parametrize("cols", SC.BATCH_WIDTHS)
def test_batch_frames(viso, oracle, cols, small):
    first, second = SC.batch_case(cols, small)
    st = MatchParams.stereo(hostmath.F_from_P(synth.KITTI_P1, synth.KITTI_P2))
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, len(first["n"]), first["cap"])
    try:
        b.set_params(st, MatchParams.temporal(), Param.kitti00(), seed=5)
        b.upload_images(first["images"], first["kp"], first["n"])
        for mode in (1, 2):
            b.set_subpixel(mode)
            b.run_images()
            lists = _check_batch(b, oracle, first, mode, "first upload")
        f, s = SC.batch_fast_counts(first, lists)
        assert (f >= 1 and s >= 1) if small else (f >= 8 and s >= 8), (f, s)
        # shorter lists on the same batch: exactly the new lengths and values, in a full run and in a matcher-only run
        b.upload_images(second["images"], second["kp"], second["n"])
        b.run_images()
        _check_batch(b, oracle, second, 2, "second upload")
        b.set_subpixel(1)
        b.run_images(matcher_only=True)
        _check_batch(b, oracle, second, 1, "second upload, matcher only")
        b.upload_images(first["images"], first["kp"], first["n"])
        b.run_images(matcher_only=True)
        _check_batch(b, oracle, first, 1, "first upload again, matcher only")
    finally:
        b.close(); ctx.close()
