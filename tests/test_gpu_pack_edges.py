"""pack_desc_kernel and pack_desc_i16_kernel at their edges, through the batch C-ABI: image sizes around the eight rows of a
wave and the 64 of a tile, image bases that leave a wave's run off 16 bytes (an odd capacity: the scalar loads), a short
descriptor, the values at and beyond the ends of int16, a flagged image beside unflagged ones, every shift of the 8-bit
planes, and the shift a counting run chooses.  The packed rows and planes have no getter; they are checked by what the
matcher kernels make of them: every list of both frames equal to the oracle's (a wrong row, plane, or a missed / spurious
flag changes SADs, bounds, or the path a problem takes)."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MatchParams

pytestmark = pytest.mark.gpu

LISTS = ((0, 0), (0, 1), (1, 1), (2, 1))


@pytest.fixture(scope="module")
def seq():
    return synth.make_sequence(91, 2, n_kp=2000, width=1241, height=376)


def _slice(seq, nk, cap=None, dlen=None):
    cap = cap or max(nk, 1)
    kp = np.zeros((2, 2, cap, 2), np.float32)
    desc = np.zeros((2, 2, cap, dlen or seq["desc"].shape[-1]), np.float32)
    kp[:, :, :nk], desc[:, :, :nk] = seq["kp"][:, :, :nk], seq["desc"][:, :, :nk, :desc.shape[-1]]
    return kp, desc, np.full((2, 2), nk, np.int32)


def _want(oracle, seq, kp, desc, n):
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    out = []
    for which, t in LISTS:
        q = (0, t) if which < 2 else (1, t)
        g = (1, t) if which == 0 else ((0, t - 1) if which == 1 else (1, t - 1))
        nq, ng = n[q[1], q[0]], n[g[1], g[0]]
        out.append(oracle.match_desc(kp[q[1], q[0], :nq], kp[g[1], g[0], :ng], desc[q[1], q[0], :nq], desc[g[1], g[0], :ng],
                                     st if which == 0 else tm))
    return out


def _run(seq, kp, desc, n, i16, shift=-1, runs=1):
    """-> (the four lists of the last run, general-path flags, the planes' shift of every run)"""
    ctx = libviso_amd.Context(0)
    libviso_amd.set_row8_shift(shift, ctx)
    b = libviso_amd.Batch(ctx, 2, kp.shape[2], desc.shape[-1])
    try:
        if i16:
            b.upload_i16(kp, np.ascontiguousarray(desc.astype(np.int16)), n)
        else:
            b.upload(kp, desc, n)
        b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=1)
        shifts = []
        for _ in range(runs):
            b.run_matcher()
            shifts.append(b.row8_shift())
            b.counters()   # (waits for the run: the next one looks at the counts this one sent back)
        return [b.matches(w, t) for w, t in LISTS], b.general_path_flags().copy(), shifts
    finally:
        b.close(); ctx.close()


def _same(got, want, tag):
    for (w, t), g, x in zip(LISTS, got, want):
        assert np.array_equal(g, x), (tag, w, t, len(g), len(x))


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("nk", [1, 7, 8, 9, 63, 64, 65, 2000])
def test_image_sizes(viso, oracle, seq, nk, i16):
    """capacity = nk: for the odd ones every image but the first starts off 16 bytes, its waves take the scalar loads."""
    kp, desc, n = _slice(seq, nk)
    got, flags, _ = _run(seq, kp, desc, n, i16)
    _same(got, _want(oracle, seq, kp, desc, n), (nk, i16))
    assert not flags.any()
    assert sum(map(len, got)) > 0 or nk < 63


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_unaligned_capacity_and_short_descriptor(viso, oracle, seq, i16):
    """capacity 301 (odd: unaligned image bases) with 300 keypoints, and 50-element descriptors (25 lanes of a row carry
    values, the others pads)."""
    for cap, dlen in ((301, None), (304, 50), (301, 50)):
        kp, desc, n = _slice(seq, 300, cap, dlen)
        got, flags, _ = _run(seq, kp, desc, n, i16)
        _same(got, _want(oracle, seq, kp, desc, n), (cap, dlen, i16))
        assert not flags.any()


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
def test_int16_end_values_stay_on_the_packed_path(viso, oracle, seq, i16):
    kp, desc, n = _slice(seq, 300)
    desc[0, 0, 3, 0], desc[0, 0, 3, 120], desc[0, 0, 11, 60] = 32767.0, -32768.0, -32767.0
    desc[1, 1, 299, 1], desc[1, 0, 8, 119] = -32768.0, 32767.0
    if not i16:
        desc[0, 1, 5, 4], desc[1, 0, 17, 120] = -0.0, -0.0
    got, flags, _ = _run(seq, kp, desc, n, i16)
    _same(got, _want(oracle, seq, kp, desc, n), i16)
    assert not flags.any()


@pytest.mark.parametrize("value", [0.5, float("nan"), 32768.0, -32769.0, 1e10, float("inf")])
@pytest.mark.parametrize("where", [(0, 0), (120, 7), (61, 299)])
def test_a_value_outside_int16_flags_its_image_only(viso, oracle, seq, value, where):
    """One element of ONE image (frame 0, left) is no int16: that image is flagged, the other three are not, and every list
    -- the two with the flagged image on the general path, the two without on the packed one, in one launch -- is the
    oracle's.  where = (element, row): first lane / last lane holding a value / a middle one; first, a wave's last, the
    image's last row."""
    e, r = where
    kp, desc, n = _slice(seq, 300)
    desc[0, 0, r, e] = value
    got, flags, _ = _run(seq, kp, desc, n, False)
    assert flags.tolist() == [[1, 0], [0, 0]], flags
    _same(got, _want(oracle, seq, kp, desc, n), (value, where))


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_every_forced_plane_shift(viso, oracle, seq, shift, i16):
    kp, desc, n = _slice(seq, 700)
    got, _, shifts = _run(seq, kp, desc, n, i16, shift=shift)
    assert shifts == [shift]
    _same(got, _want(oracle, seq, kp, desc, n), (shift, i16))


# The shift the second run takes from the first run's magnitude counts, recorded from a build of the parent commit of the
# leaner pack kernels on this very data (777 keypoints, descriptors scaled by SCALE and rounded): the counting pass reads
# the rows the wave staged, whichever loop converted them, so the sample and the choice must not move.
R8_PARENT = {0.35: 2, 0.2: 1}


@pytest.mark.parametrize("i16", [False, True], ids=["f32", "i16"])
@pytest.mark.parametrize("scale", sorted(R8_PARENT))
def test_counting_run_chooses_the_parents_shift(viso, oracle, seq, scale, i16):
    kp, desc, n = _slice(seq, 777)
    desc = np.rint(desc * scale).astype(np.float32)
    got, _, shifts = _run(seq, kp, desc, n, i16, runs=2)
    print("r8 shifts", scale, i16, shifts)
    assert shifts == [3, R8_PARENT[scale]], shifts
    _same(got, _want(oracle, seq, kp, desc, n), (scale, i16))
