"""extract_pack_kernel (csrc/extract.hip) row by row.  The kernel writes the matcher's packed u16 rows (and, for matcher
variants 5 and 6, the block sums and the 8-bit planes) and nothing reads them back; here the matcher does.  Every image
of a case carries the same keypoint positions (tests/edge_inputs.py: on, around and outside every edge the kernel
tests, at distinct half-pixel grid points) and the matchers run with radius 0.25, so the only candidate of a keypoint is
its counterpart and the row's dist is the SAD of their two packed rows: independent random images leave no wrong
descriptor element unseen.  Matches and counters must equal the oracle's (descriptors from oracle.extract_descriptors,
lists from oracle.match_desc) and be byte-equal to a feature-in batch given the oracle's descriptors, for every matcher
variant of the build and every shift of variant 6's planes.  Each case first asserts, on the oracle alone, that no probe
keypoint escapes (edge_inputs.check_probe_is_full).

Not run on the device on purpose: saturated or non-finite coordinates (the kernel clamps them before converting)."""
import numpy as np
import pytest

import libviso_amd

import edge_inputs as E

pytestmark = pytest.mark.gpu


def _run(ctx, case, st, tm, desc=None):
    b = libviso_amd.Batch(ctx, E.NF, case["cap"])
    try:
        if desc is None:
            b.upload_images(case["images"], case["kp"], case["n"])
        else:
            b.upload(case["kp"], desc, case["n"])
        b.set_params(st, tm, E.default_param(), seed=1)
        if desc is None:
            b.run_images(matcher_only=True)
        else:
            b.run_matcher()
        lists = {(w, t): b.matches(w, t) for w, t, _, _ in E.problems()}
        sc, mo = b.counters()
    finally:
        b.close()
    return lists, sc, mo


def _check(oracle, shape, counts, kind="random"):
    st, tm = E.match_params()
    ctx = libviso_amd.Context(0)
    try:
        for pad in E.CAP_PADS:
            case = E.extract_case(shape, counts, pad, kind)
            desc, want = E.extract_expected(oracle, case)
            E.check_probe_is_full(case, want)                      # the condition, on the oracle alone, first
            w_sc = np.zeros((3, E.NF), np.int64)
            w_mo = np.zeros((3, E.NF), np.int64)
            for (w, t), (m, scored) in want.items():
                w_sc[w, t], w_mo[w, t] = scored, len(m)
            for variant, shift in E.matcher_configs(libviso_amd.matcher_variants()):
                tag = (shape, np.asarray(counts).tolist(), case["cap"], kind, variant, shift)
                libviso_amd.set_matcher_variant(variant, ctx)
                libviso_amd.set_row8_shift(shift, ctx)
                got, sc, mo = _run(ctx, case, st, tm)
                for k, (m, _) in want.items():
                    assert np.array_equal(got[k], m), (tag, k)
                assert np.array_equal(sc, w_sc) and np.array_equal(mo, w_mo), tag
                ref, sc2, mo2 = _run(ctx, case, st, tm, desc)
                for k in want:
                    assert got[k].tobytes() == ref[k].tobytes(), (tag, k)
                assert sc.tobytes() == sc2.tobytes() and mo.tobytes() == mo2.tobytes(), tag
    finally:
        ctx.close()


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("count", E.COUNTS, ids=_ids)
@pytest.mark.parametrize("shape", E.SHAPES, ids=_ids)
def test_packed_rows_at_every_edge(viso, oracle, shape, count):
    _check(oracle, shape, count)


@pytest.mark.parametrize("count", E.EXTRA_COUNTS, ids=_ids)
def test_packed_rows_totals_of_the_wave_tails(viso, oracle, count):
    """Images of 1, 3, 5, 64 and 257 keypoints in all (the sentinel included)."""
    _check(oracle, E.SHAPES[0], count)


@pytest.mark.parametrize("shape", [E.SHAPES[0], E.SHAPES[1]], ids=_ids)
def test_packed_rows_ragged_counts(viso, oracle, shape):
    _check(oracle, shape, E.RAGGED_COUNTS)


def test_packed_rows_full_plane_range(viso, oracle):
    """Columns of 0 and 255: Sobel-x reaches +-1020, the ends of the u16 rows' bias and of every plane shift's clamp."""
    _check(oracle, E.SHAPES[0], 65, kind="columns")
