"""The device helpers of wave.h, match_dev.h, voxel_hash.h and solver_dev.h called directly, lane by lane, through the test-only
harness (tests/dev_harness/helpers.hip, built with the library's flags by tests/dev_harness.py), against the numpy lane models of
tests/wave_ref.py, plain numpy / Python integer restatements, and the oracle.  Every comparison is bit for bit: integer arithmetic,
or IEEE add / mul / div under -ffp-contract=off.  Whole waves only (the headers exclude anything else); every probe loop under test
is bounded by construction."""
import itertools

import numpy as np
import pytest

import dev_harness as H
import wave_ref as W
from libviso_amd.abi import Param

pytestmark = pytest.mark.gpu

EDGE_LANES = (0, 15, 16, 31, 32, 47, 48, 63)
U32, U64, F32, F64, I32 = np.uint32, np.uint64, np.float32, np.float64, np.int32
M64 = (1 << 64) - 1


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(got, want, what=""):
    got, want = bits(got), bits(want)
    bad = np.nonzero(got != want)
    assert bad[0].size == 0, (what, [int(b[0]) for b in bad], got[bad][:4], want[bad][:4])


def per_wave(model, *arrays):
    """model over every 64 lanes of the arrays (first axis)."""
    n = len(arrays[0])
    return np.concatenate([np.asarray(model(*(a[w:w + 64] for a in arrays))) for w in range(0, n, 64)])


def distinct_u32(n, seed=1):
    """Lane-distinct values: no two of the n are equal, so a wrong source lane cannot pass."""
    return ((np.arange(n, dtype=U64) + U64(seed)) * U64(0x9E3779B1) % U64(1 << 32)).astype(U32)


def distinct_u64(n, seed=1):
    return (np.arange(n, dtype=U64) + U64(seed)) * U64(0x9E3779B97F4A7C15)


def pad256(a):
    """First axis up to a multiple of 256, by repeating the last row."""
    k = -len(a) % 256
    return np.ascontiguousarray(np.concatenate([a, np.repeat(a[-1:], k, axis=0)]) if k else a)


# ---- wave.h: lane moves -------------------------------------------------------------------------------------------------------------

def test_dpp_moves_read_the_documented_lane():
    """wave_dpp (old = 0, kept), wave_dpp_bc (bound_ctrl: 0) and viso_dpp (old = ident, row mask) for every control and row mask
    that occurs in the library: the source lane's value, and in a lane without a source, or in a row outside the mask, the
    documented one."""
    n = 2048
    v, ident = distinct_u32(n), distinct_u32(n, 77777)
    for name in H.ELEMENTWISE:
        if name.startswith("wave_dpp_bc_"):
            ctrl = int(name.rsplit("_", 1)[1], 16)
            want = per_wave(lambda x: W.dpp(x, ctrl, 0xF, 0, bound_ctrl=True), v)
            got = H.call(name, np.full(n, 0xCCCCCCCC, U32), v)
        elif name.startswith("wave_dpp_"):
            ctrl = int(name.rsplit("_", 1)[1], 16)
            want = per_wave(lambda x: W.dpp(x, ctrl, 0xF, 0), v)
            got = H.call(name, np.full(n, 0xCCCCCCCC, U32), v)
        elif name.startswith("viso_dpp_"):
            ctrl, mask = (int(t, 16) for t in name.split("_")[2:])
            want = per_wave(lambda x, o: W.dpp(x, ctrl, mask, o), v, ident)      # the lane's own ident where nothing arrives
            got = H.call(name, np.full(n, 0xCCCCCCCC, U32), v, ident)
        else:
            continue
        same_bits(got, want, name)


def test_dpp_f64_moves_both_halves():
    n = 1024
    v = distinct_u64(n).view(F64)
    for ctrl, mask in W.WAVE_STEPS:
        got = H.call("dpp_f64_0x%x_0x%x" % (ctrl, mask), np.full(n, 7.0), v)
        same_bits(got, per_wave(lambda x: W.dpp(bits(x), ctrl, mask, 0), v), hex(ctrl))   # no source, outside the mask: 0.0


def test_wave_shifts_and_swizzles():
    n = 1024
    v = distinct_u32(n)
    same_bits(H.call("wave_shr1", np.ones(n, F32), v.view(F32)), per_wave(lambda x: W.dpp(x, 0x138, 0xF, 0, True), v), "shr1")
    same_bits(H.call("wave_shl1", np.ones(n, F32), v.view(F32)), per_wave(lambda x: W.dpp(x, 0x130, 0xF, 0, True), v), "shl1")
    lane = np.arange(n)
    same_bits(H.call("wave_swizzle_0x101F", np.zeros(n, U32), v), v[lane ^ 4], "lane ^ 4")
    same_bits(H.call("wave_swizzle_0x401F", np.zeros(n, U32), v), v[lane ^ 16], "lane ^ 16")
    d = distinct_u64(n).view(F64)
    got = H.call("swz_bcast8", np.zeros((n, 8)), d)
    for i in range(8):
        same_bits(got[:, i], d[(lane & ~7) | i], "swz_bcast8<%d>" % i)


def test_lane_reads():
    """bperm (every source lane, in and out of order), rdlane (constant lane), readlane_f32 (wave-uniform lane), uni."""
    n = 4096                                 # 64 waves
    rng = np.random.default_rng(3)
    d = distinct_u64(n).view(F64)
    lane, base = np.arange(n) & 63, np.arange(n) & ~63
    for src in (lane, 63 - lane, (lane * 5 + 3) & 63, np.repeat(np.arange(64), 64), rng.integers(0, 64, n)):
        src = np.ascontiguousarray(src, I32)
        same_bits(H.call("bperm", np.zeros(n), d, src), d[base + src], "bperm")
    got = H.call("rdlane", np.zeros((n, 8)), d)
    for col, k in enumerate(EDGE_LANES):
        same_bits(got[:, col], d[base + k], "rdlane %d" % k)
    f = distinct_u32(n).view(F32)
    k = np.ascontiguousarray(np.repeat(rng.permutation(64), 64), I32)        # wave w reads lane k[w]: every lane once
    same_bits(H.call("readlane_f32", np.zeros(n, F32), f, k), f[base + k], "readlane_f32")
    same_bits(H.call("uni", np.zeros(n), d), d[base], "uni")


# ---- wave.h: reductions and scans ---------------------------------------------------------------------------------------------------

def _u32_waves():
    rng = np.random.default_rng(11)
    w = [rng.integers(0, 2 ** 32, 64, dtype=U64).astype(U32) for _ in range(6)]
    w += [np.full(64, 5, U32), np.zeros(64, U32), np.full(64, 0xFFFFFFFF, U32)]            # all equal; the identities as data
    for lane in EDGE_LANES:
        lo = rng.integers(1000, 2 ** 31, 64).astype(U32)
        lo[lane] = 3                                                                       # the minimum in one lane
        hi = rng.integers(1000, 2 ** 31, 64).astype(U32)
        hi[lane] = 0xFFFFFFF0                                                              # the maximum
        ident = np.full(64, 0xFFFFFFFF, U32)
        ident[lane] = 0                                                                    # identities on both sides
        w += [lo, hi, ident, ~ident]
    return pad256(np.concatenate(w))


def test_u32_reductions_and_scans():
    v = _u32_waves()
    n = len(v)
    last = np.arange(63, n, 64)
    rows = v.reshape(-1, 16)
    wmin, wmax = v.reshape(-1, 64).min(axis=1), v.reshape(-1, 64).max(axis=1)
    for name, want63, model in (("wave_min63", wmin, W.wave_min63), ("wave_max63", wmax, W.wave_max63)):
        got = H.call(name, np.zeros(n, U32), v)
        assert np.array_equal(got[last], want63), name                                     # valid in lane 63
        assert np.array_equal(got[last], per_wave(model, v)[last]), name
    got = H.call("wave_scan", np.zeros(n, U32), v)                                          # every lane, not only 63
    assert np.array_equal(got, np.concatenate([np.cumsum(w, dtype=U32) for w in v.reshape(-1, 64)]))
    assert np.array_equal(got, per_wave(W.wave_scan, v))
    assert np.array_equal(H.call("wave_min_u32", np.zeros(n, U32), v), np.repeat(wmin, 64))   # to every lane
    assert np.array_equal(H.call("wave_max_u32", np.zeros(n, U32), v), np.repeat(wmax, 64))
    assert np.array_equal(H.call("row_min_u32", np.zeros(n, U32), v), np.repeat(rows.min(axis=1), 16))
    assert np.array_equal(H.call("group_sum_4", np.zeros(n, U32), v), np.repeat(v.reshape(-1, 4).sum(axis=1, dtype=U32), 4))
    assert np.array_equal(H.call("group_sum_8", np.zeros(n, U32), v), np.repeat(v.reshape(-1, 8).sum(axis=1, dtype=U32), 8))


def _u64_waves():
    rng = np.random.default_rng(12)
    w = [rng.integers(0, 2 ** 63, 64, dtype=U64) * U64(2) + U64(1) for _ in range(4)]
    w += [np.full(64, 9, U64), np.zeros(64, U64), np.full(64, M64, U64)]
    for lane in EDGE_LANES:
        hi = rng.integers(10, 1000, 64).astype(U64)
        k = (hi << U64(32)) | rng.integers(0, 2 ** 32, 64, dtype=U64)
        k[lane] = (U64(5000) << U64(32)) | U64(1)                  # the maximal high word, a small low word; larger low words elsewhere
        w.append(k)
        tie = (U64(77) << U64(32)) | rng.integers(0, 2 ** 31, 64, dtype=U64)      # a tie in the high word, the low word decides
        tie[lane] = (U64(77) << U64(32)) | U64(0xFFFFFFFE)
        tie[(lane + 9) & 63] = (U64(76) << U64(32)) | U64(0xFFFFFFFF)             # a lower high word with the largest low word
        w.append(tie)
        low0 = rng.integers(0, 50, 64).astype(U64) << U64(32)                     # low words 0
        low0[lane] = U64(50) << U64(32)
        w.append(low0)
        carry = rng.integers(0, 2 ** 32, 64, dtype=U64) | U64(0xFFFF0000)        # 32-bit halves that carry into the high word
        carry[lane] |= U64(0xFFFFFFFF) << U64(32)                                  # and out of it (the sum wraps)
        w.append(carry)
    return pad256(np.concatenate(w))


def test_u64_reductions():
    k = _u64_waves()
    n = len(k)
    last = np.arange(63, n, 64)
    kw = k.reshape(-1, 64)
    assert np.array_equal(H.call("wave_max63_u64", np.zeros(n, U64), k)[last], kw.max(axis=1))
    assert np.array_equal(H.call("wave_max_u64", np.zeros(n, U64), k), np.repeat(kw.max(axis=1), 64))     # to every lane
    assert np.array_equal(H.call("wave_sum63", np.zeros(n, U64), k)[last], kw.sum(axis=1, dtype=U64))
    assert np.array_equal(per_wave(W.wave_max_u64, k), np.repeat(kw.max(axis=1), 64))


def _fext_waves():
    rng = np.random.default_rng(13)
    nan, inf = np.nan, np.inf
    w = []
    for lane in EDGE_LANES:
        a = rng.normal(0, 100, 64).astype(F32)
        a[lane] = -1e30
        b = rng.normal(0, 100, 64).astype(F32)
        b[lane] = 1e30
        c = rng.normal(0, 100, 64).astype(F32)
        c[lane] = nan                                            # NaN in one lane
        d = np.full(64, nan, F32)
        d[lane] = 2.5                                            # NaN in all lanes but one
        e = np.zeros(64, F32)
        e[lane] = -0.0                                           # +-0 only
        f = rng.normal(0, 100, 64).astype(F32)
        f[lane], f[(lane + 5) & 63] = inf, -inf
        w += [a, b, c, d, e, f]
    w += [np.full(64, nan, F32), np.full(64, -0.0, F32), np.full(64, 1.5, F32), np.full(64, inf, F32), np.full(64, -inf, F32)]
    return pad256(np.concatenate(w))


@pytest.mark.parametrize("is_max", [False, True])
def test_wave_fext(is_max):
    """Minimum / maximum of a float to every lane: NaN operands are ignored (NaN only from a wave of NaN); where zeros of both signs
    tie the header promises no sign."""
    v = _fext_waves()
    got = H.call("wave_fext_max" if is_max else "wave_fext_min", np.zeros(len(v), F32), v)
    with np.errstate(all="ignore"):
        ref = np.repeat((np.nanmax if is_max else np.nanmin)(np.where(np.isnan(v).reshape(-1, 64).all(axis=1, keepdims=True), 0,
                                                                      v.reshape(-1, 64)), axis=1), 64).astype(F32)
    allnan = np.repeat(np.isnan(v).reshape(-1, 64).all(axis=1), 64)
    assert np.isnan(got[allnan]).all() and not np.isnan(got[~allnan]).any()
    zero = ~allnan & (ref == 0)
    assert (got[zero] == 0).all()
    same_bits(got[~allnan & ~zero], ref[~allnan & ~zero])
    model = per_wave(lambda x: W.wave_fext(x, is_max), v)
    assert np.array_equal(model[~allnan], ref[~allnan])


# ---- wave.h: float sums (the order of the additions is part of the contract) ------------------------------------------------------------

def test_float_sums_in_the_documented_order():
    rng = np.random.default_rng(14)
    n = 2048
    f = (rng.normal(0, 1, n) * 10.0 ** rng.uniform(-6, 6, n)).astype(F32)
    f[:64] = 0
    f[0], f[1], f[2] = 1e8, 1.0, -1e8                          # a cancellation that another order of additions keeps
    last = np.arange(63, n, 64)
    same_bits(H.call("wave_fsum63", np.zeros(n, F32), f)[last], per_wave(W.wave_scan, f)[last], "fsum63")
    d = rng.normal(0, 1, n) * 10.0 ** rng.uniform(-9, 9, n)
    d[:64] = 0
    d[0], d[1], d[2] = 1e17, 1.0, -1e17
    same_bits(H.call("wave_sum_to_lane63", np.zeros(n), d)[last], per_wave(W.wave_scan, d)[last], "wave_sum_to_lane63")


@pytest.mark.parametrize("ns", [7, 27, 50])
def test_block_sum(ns):
    """block_sum<NS, 4> as refine.hip (7, 27) and covariance.hip (50) instantiate it: every thread returns with the same tot[]."""
    rng = np.random.default_rng(ns)
    n = 768                                                    # three workgroups
    acc = np.ascontiguousarray(rng.normal(0, 1, (n, ns)) * 10.0 ** rng.uniform(-8, 8, (n, ns)))
    got = H.call("block_sum_%d_4" % ns, np.zeros((n, ns)), acc)
    for blk in range(n // 256):
        want = W.block_sum(acc[blk * 256:(blk + 1) * 256], 4)
        same_bits(got[blk * 256:(blk + 1) * 256], np.tile(want, (256, 1)), "block %d" % blk)


# ---- wave.h: one-instruction helpers --------------------------------------------------------------------------------------------------

SPECIAL_F32 = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.17549435e-38, 1.5, -2.25, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan], F32)


def test_abs_adds():
    a, b = (pad256(x.ravel()) for x in np.meshgrid(SPECIAL_F32, SPECIAL_F32))
    c = np.ascontiguousarray(np.roll(a, 3))
    with np.errstate(all="ignore"):
        want2 = np.abs(a) + np.abs(b)
        want3 = (c + np.abs(a)) + np.abs(b)
    for got, want in ((H.call("abs_add_abs", np.zeros(len(a), F32), a, b), want2), (H.call("add_abs_abs", np.zeros(len(a), F32), c, a, b), want3)):
        nan = np.isnan(want)
        assert np.isnan(got[nan]).all()
        same_bits(got[~nan], want[~nan])


@pytest.mark.parametrize("name", ["fmin_raw", "fmax_raw"])
def test_raw_min_max(name):
    """v_min / v_max as fminf / fmaxf do them: a quiet NaN operand gives the OTHER operand, bit for bit (denormals included);
    min(-0, +0): a zero, no sign promised."""
    a, b = (pad256(x.ravel()) for x in np.meshgrid(SPECIAL_F32, SPECIAL_F32))
    got = H.call(name, np.zeros(len(a), F32), a, b)
    an, bn = np.isnan(a), np.isnan(b)
    assert np.isnan(got[an & bn]).all()
    same_bits(got[an & ~bn], b[an & ~bn], "NaN a")
    same_bits(got[~an & bn], a[~an & bn], "NaN b")
    both = ~an & ~bn
    zeros = both & (a == 0) & (b == 0)
    assert (got[zeros] == 0).all()
    want = (np.minimum if name == "fmin_raw" else np.maximum)(a, b)
    same_bits(got[both & ~zeros], want[both & ~zeros], "ordered")


def test_med3_u32():
    vals = [0, 1, 2, 3, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]          # unsigned: the high bit is no sign
    trip = np.array(list(itertools.product(vals, repeat=3)), U32)             # all six orderings of every triple, and every tie
    a, b, c = (pad256(np.ascontiguousarray(trip[:, i])) for i in range(3))
    got = H.call("med3_u32", np.zeros(len(a), U32), a, b, c)
    assert np.array_equal(got, np.sort(np.stack([a, b, c]), axis=0)[1])


# ---- match_dev.h ----------------------------------------------------------------------------------------------------------------------

def test_row8_forms_agree_with_the_clamp_and_shift():
    """row8_of, row8_of_uniform and row8_pair_of_biased against clip(v + (128 << s), 0, (256 << s) - 1) >> s: every int16 at every
    shift, values outside int16 for the two row8_of forms."""
    v16 = np.arange(-32768, 32768, dtype=I32)
    wide = np.array([-2 ** 30, -100000, -40000, -32769, 32768, 40000, 100000, 2 ** 30], I32)
    v = pad256(np.concatenate([v16, wide]))
    lo = (v16 + 32768).astype(U32)
    hi = (lo * U32(40503) + U32(12345)) & U32(0xFFFF)            # a bijection of the 16-bit values: every value in the upper half too
    row = np.ascontiguousarray(lo | (hi << U32(16)))
    for s in range(4):
        want = W.row8(v, s)
        assert np.array_equal(H.call("row8_of", np.zeros(len(v), U32), v, np.full(len(v), s, I32)), want), s
        assert np.array_equal(H.call("row8_of_uniform", np.zeros(len(v), U32), v, p=s), want), s
        pair = W.row8(lo.astype(np.int64) - 32768, s) | (W.row8(hi.astype(np.int64) - 32768, s) << U32(8))
        assert np.array_equal(H.call("row8_pair_of_biased", np.zeros(len(row), U32), row, p=s), pair), s
    s = np.ascontiguousarray(np.arange(len(v)) & 3, I32)         # row8_of takes a shift per lane
    assert np.array_equal(H.call("row8_of", np.zeros(len(v), U32), v, s), np.choose(s, [W.row8(v, k) for k in range(4)]))


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_store_row8_writes_its_row_and_nothing_else(mode):
    """store_row8_pair / store_row8<false> / store_row8<true>: the 128 bytes of the wave's row; the rows on both sides of it (guards
    of 0xA5) stay untouched."""
    rng = np.random.default_rng(20 + mode)
    n = 512
    for s in range(4 if mode else 1):
        va = rng.integers(-1500, 1500, n).astype(I32)
        vb = rng.integers(-1500, 1500, n).astype(I32)
        if mode == 0:
            va = rng.integers(0, 65536, n).astype(I32)           # h2: the lane's two plane bytes
            b0, b1 = va & 255, va >> 8
        else:
            b0, b1 = W.row8(va, s), W.row8(vb, s)
        buf = H.store_row8(np.full((2 * (n // 64) + 1) * 128, 0xA5, np.uint8), va, vb, s, mode).reshape(-1, 128)
        assert (buf[0::2] == 0xA5).all(), (mode, s)
        want = np.stack([b0, b1], axis=1).reshape(n // 64, 128).astype(np.uint8)
        assert np.array_equal(buf[1::2], want), (mode, s)


def test_pack_block_sums_clamps_every_block_on_its_own():
    rng = np.random.default_rng(21)
    targets = [-100000, -40000, -32769, -32768, -32767, -1, 0, 1, 32766, 32767, 32768, 40000, 100000]
    waves = []
    for t in range(len(targets) * 2):
        w = rng.integers(-300, 300, 64)
        for blk in range(4):                                     # a different sum in each of the four 16-lane blocks
            want = targets[(t + 3 * blk) % len(targets)]
            w[blk * 16 + int(rng.integers(16))] += want - w[blk * 16:(blk + 1) * 16].sum()
        waves.append(w)
    v = pad256(np.concatenate(waves).astype(I32))
    got = H.call("pack_block_sums", np.zeros((len(v), 2), U32), v)
    want = np.array([W.pack_block_sums(w) for w in v.reshape(-1, 64)], U32)
    assert np.array_equal(got, np.repeat(want, 64, axis=0))      # valid in every lane
    sums = v.reshape(-1, 16).sum(axis=1)
    assert (sums < -32768).any() and (sums > 32767).any() and (sums == 32767).any() and (sums == -32768).any()


def test_mbcnt():
    rng = np.random.default_rng(22)
    n = 2048
    lane = np.arange(n) & 63
    m = rng.integers(0, 2 ** 63, n, dtype=U64) * U64(2) + rng.integers(0, 2, n).astype(U64)
    m[:64], m[64:128] = 0, M64
    for i, b in enumerate((0, 31, 32, 63)):
        m[128 + 64 * i:192 + 64 * i] = U64(1) << U64(b)
    got = H.call("mbcnt", np.zeros(n, I32), m)
    want = [bin(int(x) & ((1 << int(l)) - 1)).count("1") for x, l in zip(m, lane)]
    assert np.array_equal(got, np.array(want, I32))


def test_l1_bits_is_l1_kp():
    rng = np.random.default_rng(23)
    n = 2048
    q = rng.uniform(-2000, 2000, (n, 4)).astype(F32)
    q[:256, 2:] = q[:256, :2]                                    # differences of +0
    q[256:512, 2] = q[256:512, 0]
    q[256:512, 3] = np.nextafter(q[256:512, 1], F32(np.inf))
    sp = np.array(list(itertools.product([0.0, -0.0, np.inf, -np.inf, 1e-42, 3.0], repeat=4)), F32)   # -0.0 differences, infinities
    q[512:512 + len(sp)] = sp
    got = H.call("l1", np.zeros((n, 2), U32), q)
    with np.errstate(all="ignore"):
        want = np.abs(q[:, 0] - q[:, 2]) + np.abs(q[:, 1] - q[:, 3])
    nan = np.isnan(want)
    assert nan.any() and np.isnan(got[nan].view(F32)).all()      # (inf - inf: a NaN on both sides; which NaN is not a property of IEEE)
    assert np.array_equal(got[~nan, 0], got[~nan, 1])
    assert np.array_equal(got[~nan, 0], bits(want)[~nan])


def _bucket_inputs(nb):
    rng = np.random.default_rng(24)
    inf, nan = np.inf, np.nan
    cases = []
    sweep = np.sort(np.concatenate([rng.uniform(-500, 3000, 700), [-inf, inf, -3e38, 3e38, 0.0, -0.0, 1241.0], np.arange(0, 1241, 0.5)])).astype(F32)
    for x0, scale in ((0.0, nb / 1241.0), (-37.5, nb / 50.0), (100.0, 0.0), (0.0, 3e9), (-inf, 1.0), (5.0, 1e-30), (0.0, 1e38)):
        cases.append(np.stack([sweep, np.full_like(sweep, x0), np.full_like(sweep, scale)], axis=1))
    odd = [(nan, 0.0, 1.0), (nan, inf, 0.0), (nan, 0.0, 0.0), (inf, 0.0, 0.0), (-inf, 0.0, 0.0), (1.0, inf, 0.0), (1.0, -inf, 0.0), (inf, inf, 1.0),
           (-inf, -inf, 1.0), (1.0, inf, 1.0), (3e38, -3e38, 2.0), (5.0, 0.0, 1e30), (-5.0, 0.0, 1e30), (2.0 ** 31, 0.0, 1.0), (-2.0 ** 31 - 512, 0.0, 1.0)]
    cases.append(np.array(odd, F32))
    a = np.concatenate(cases).astype(F32)
    with np.errstate(all="ignore"):
        prod = (a[:, 0] - a[:, 1]) * a[:, 2]
    # bucket_of_finite is fed a NaN x, or a product that is a number: its (int)NaN is the one thing its comment excludes
    w = (np.isnan(a[:, 0]) | ~np.isnan(prod)).astype(F32)
    return pad256(np.concatenate([a, w[:, None]], axis=1)), len(sweep), len(cases) - 1


@pytest.mark.parametrize("nb", [256, 64])
def test_bucket_maps_are_monotone_total_and_agree(nb):
    """bucket_of, bucket_of_finite and bucket_cvt for VISO_NB = 256 and for the 64 of ST_NBY and MU_NBY: inside [0, NB), monotone over
    a sorted sweep (+-inf at its ends), equal to each other except at a NaN x (bucket_of: the last bucket, bucket_cvt: 0), and
    bucket_of equal to its float32 restatement."""
    a, ns, nsweeps = _bucket_inputs(nb)
    got = H.call("buckets", np.zeros((len(a), 3), I32), a, p=nb)
    of, cvt, fin = got[:, 0], got[:, 1], got[:, 2]
    assert of.min() >= 0 and of.max() < nb and cvt.min() >= 0 and cvt.max() < nb
    xnan, fed = np.isnan(a[:, 0]), a[:, 3] != 0
    assert xnan.any() and (of[xnan] == nb - 1).all() and (cvt[xnan] == 0).all() and (fin[xnan] == nb - 1).all()
    assert np.array_equal(of[~xnan], cvt[~xnan])
    assert np.array_equal(fin[fed], of[fed]) and (fin[~fed] == -1).all() and (~fed).any()
    for k in range(nsweeps):
        for col in (of, cvt):
            assert (np.diff(col[k * ns:(k + 1) * ns]) >= 0).all(), k
    assert len(np.unique(of[:ns])) == nb                          # the first sweep spans every bucket
    with np.errstate(all="ignore"):
        f = np.floor((a[:, 0] - a[:, 1]) * a[:, 2])
    want = np.where(xnan, nb - 1, np.where(np.isnan(f), 0, np.clip(np.nan_to_num(f, nan=0.0), 0, nb - 1))).astype(I32)
    assert np.array_equal(of, want)


def _bitonic_rows(rng, npad, guard):
    rows = [rng.integers(0, 2 ** 63, npad, dtype=U64),                                   # random
            np.full(npad, 0x0123456789ABCDEF, U64),                                      # all equal
            np.sort(rng.integers(0, 2 ** 63, npad, dtype=U64)),                          # sorted
            np.sort(rng.integers(0, 2 ** 63, npad, dtype=U64))[::-1],                    # reversed
            np.where(np.arange(npad) < (npad * 5) // 8 + 1, rng.integers(0, 2 ** 63, npad, dtype=U64), U64(M64)),   # ~0 padding
            rng.integers(0, 7, npad).astype(U64) << U64(32) | rng.integers(0, 3, npad).astype(U64)]               # duplicate keys
    g = U64(0xA5A5A5A500000000) + np.arange(guard, dtype=U64)
    return np.ascontiguousarray(np.stack([np.concatenate([r, g]) for r in rows])), g


@pytest.mark.parametrize("threads", [512, 256])
def test_bitonic_sort_lds_sorts_and_stays_inside_npad(threads):
    """npad = 64 .. VISO_SORT_MAX, one workgroup per input kind.  The sort gets npad keys of an LDS array that goes on behind them
    with a guard pattern (npad more keys; 2048 where twice npad keys do not fit the LDS): an overrun lands inside the allocation
    and is seen."""
    rng = np.random.default_rng(threads)
    npad = 64
    while npad <= 16384:
        guard = npad if npad <= 8192 else 2048
        io, g = _bitonic_rows(rng, npad, guard)
        want = np.sort(io[:, :npad], axis=1)
        H.bitonic(io, npad, threads)
        assert np.array_equal(io[:, npad:], np.tile(g, (len(io), 1))), ("keys behind npad were written", npad)
        assert np.array_equal(io[:, :npad], want), npad
        npad <<= 1


def sampson_np(F, p1, p2):
    """sampson_dev restated with its roundings: double sums of float coordinates, the algebraic distance rounded to float and squared
    in float, divided in double."""
    F = np.asarray(F, F64).reshape(-1, 9)
    p1x, p1y, p2x, p2y = (np.asarray(c, F32) for c in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]))
    a0, a1, b0, b1 = (c.astype(F64) for c in (p1x, p1y, p2x, p2y))
    f = [F[:, i] for i in range(9)]
    with np.errstate(all="ignore"):
        Fx0 = f[0] * a0 + f[1] * a1 + f[2]
        Fx1 = f[3] * a0 + f[4] * a1 + f[5]
        Ftx0 = f[0] * b0 + f[3] * b1 + f[6]
        Ftx1 = f[1] * b0 + f[4] * b1 + f[7]
        adv = (b0 * f[0] * a0 + b0 * f[1] * a1 + b0 * f[2] * 1.0 + b1 * f[3] * a0 + b1 * f[4] * a1 + b1 * f[5] * 1.0 + 1.0 * f[6] * a0 +
               1.0 * f[7] * a1 + 1.0 * f[8] * 1.0)
        ad = adv.astype(F32)
        ad2 = ad * ad
        return ad2.astype(F64) / (Fx0 * Fx0 + Fx1 * Fx1 + Ftx0 * Ftx0 + Ftx1 * Ftx1)


def band_np(F, thresh, xa, xb, ya, yb, r):
    """epipolar_band restated in double (one case): used to choose the generator below, and reported against the device."""
    inf = np.inf
    if not (thresh >= 0 and r >= 0 and xa <= xb and ya <= yb):
        return inf
    x, y = (float(xa), float(xb)), (float(ya), float(yb))
    X, Y = max(abs(x[0]), abs(x[1])), max(abs(y[0]), abs(y[1]))
    f0 = [F[0] * xi + F[1] * yj + F[2] for xi in x for yj in y]
    f1 = [F[3] * xi + F[4] * yj + F[5] for xi in x for yj in y]
    M0, M1, m1 = max(map(abs, f0)), max(map(abs, f1)), min(map(abs, f1))
    if any(v > 0 for v in f1) and any(v < 0 for v in f1):
        m1 = 0.0
    A = np.abs(F)
    S0, S1 = A[0] * X + A[1] * Y + A[2], A[3] * X + A[4] * Y + A[5]
    m1 -= 1e-9 * S1
    M0 += 1e-9 * S0
    M1 += 1e-9 * S1
    if not m1 > 0:
        return inf
    Xt, Yt = X + float(r), Y + float(r)
    N0, N1 = A[0] * Xt + A[3] * Yt + A[6], A[1] * Xt + A[4] * Yt + A[7]
    G = (A[0] * X * X + abs(F[1] + F[3]) * X * Y + A[4] * Y * Y + abs(F[2] + F[6]) * X + abs(F[5] + F[7]) * Y + A[8] +
         1e-9 * ((A[1] + A[3]) * X * Y + (A[2] + A[6]) * X + (A[5] + A[7]) * Y))
    T = Xt * (A[0] * X + A[1] * Y + A[2]) + Yt * (A[3] * X + A[4] * Y + A[5]) + A[6] * X + A[7] * Y + A[8]
    D = M0 * M0 + M1 * M1 + N0 * N0 + N1 * N1
    with np.errstate(all="ignore"):
        if not np.sqrt(thresh * D) >= 1e-18:
            return inf
        Emin = (np.sqrt(thresh * D) * (1.0 + 2e-6) + 1e-9 * T) * (1.0 + 2e-6)
        band = ((Emin + float(r) * M0 + G) / m1) * (1.0 + 1e-6) + 1e-6
    if not band == band or band > 3.0e38:
        return inf
    bf = F32(band)
    return bf if float(bf) >= band else np.nextafter(bf, F32(inf))


def band_cases(oracle, n=512):
    """F of every kind of tests/test_gpu_fuzz.py (its _random_F), query boxes of a tile's size inside a KITTI image, radii of the
    stereo call's order: (F [n, 9], thresh [n], box and radius [n, 5] float32)."""
    from test_gpu_fuzz import _random_F
    rng = np.random.default_rng(25)
    Fs, th, box = [], [], []
    for _ in range(n):
        Fs.append(np.asarray(_random_F(rng, oracle), F64).reshape(9))
        th.append(float(rng.choice([0.25, 1.0, 4.0])))
        xa, ya = rng.uniform(0, 1200), rng.uniform(0, 350)
        w, h = rng.choice([0.0, 8.0, 40.0]), rng.choice([0.0, 4.0, 20.0])
        box.append((xa, xa + w, ya, ya + h, float(rng.choice([100.0, 200.0, 400.0]))))
    return np.array(Fs), np.array(th), np.array(box, F32)


def test_epipolar_band_culls_only_what_the_gate_rejects(oracle):
    """Every candidate within L1 distance r of a query of the box whose |dy| is one float above the band fails the gate of
    sampson_dev (value > thresh, or not finite).  sampson_dev itself is compared with its restatement first."""
    Fs, th, box = band_cases(oracle)
    n = len(Fs)
    band = H.call("epipolar_band", np.zeros(n, F32), np.ascontiguousarray(np.c_[Fs, th]), box)
    restated = np.array([band_np(Fs[i], th[i], *box[i]) for i in range(n)], F32)
    print("device band == restated band in %d of %d cases" % (int((bits(band) == bits(restated)).sum()), n))
    r = box[:, 4]
    usable = np.isfinite(band) & (band < r)
    print("finite band below r: %d of %d cases" % (int(usable.sum()), n))
    assert usable.sum() * 2 >= n
    rng = np.random.default_rng(26)
    reps = 16
    idx = np.repeat(np.nonzero(usable)[0], reps)
    m = len(idx)
    cx = rng.integers(0, 3, m) / 2.0                              # queries: the box's corners, edge midpoints and centre
    cy = rng.integers(0, 3, m) / 2.0
    p1 = np.stack([box[idx, 0] + cx * (box[idx, 1] - box[idx, 0]), box[idx, 2] + cy * (box[idx, 3] - box[idx, 2])], axis=1).astype(F32)
    sign = rng.choice([-1.0, 1.0], m).astype(F32)
    dy = np.nextafter(band[idx], F32(np.inf))
    p2y = (p1[:, 1] + sign * dy).astype(F32)
    for _ in range(4):                                            # the float p2.y - p1.y itself must exceed the band
        short = np.abs(p2y.astype(F64) - p1[:, 1]) <= band[idx]
        p2y = np.where(short, np.nextafter(p2y, (sign * np.inf).astype(F32)), p2y).astype(F32)
    ady = np.abs(p2y.astype(F64) - p1[:, 1])
    assert (ady > band[idx]).all()
    room = r[idx] - ady                                           # |dx| + |dy| <= r
    dx = (rng.uniform(-1, 1, m) * np.maximum(room, 0) * (1 - 1e-6)).astype(F32)
    dx[::4] = 0
    p2 = np.stack([(p1[:, 0] + dx).astype(F32), p2y], axis=1)
    keep = (np.abs(p2[:, 0].astype(F64) - p1[:, 0]) + ady <= r[idx]) & (room > 0)
    assert keep.sum() >= 8 * usable.sum()
    idx, p1, p2 = idx[keep], p1[keep], p2[keep]
    k = pad256(np.arange(len(idx)))
    dev = H.call("sampson", np.zeros(len(k)), np.ascontiguousarray(Fs[idx][k]), np.ascontiguousarray(np.c_[p1, p2][k].astype(F32)))[:len(idx)]
    val = sampson_np(Fs[idx], p1, p2)
    nan = np.isnan(val)
    assert np.isnan(dev[nan]).all()
    same_bits(dev[~nan], val[~nan], "sampson_dev against its restatement")
    passes = np.isfinite(val) & ~(val > th[idx])
    assert not passes.any(), (int(passes.sum()), idx[passes][:5], val[passes][:5], band[idx[passes]][:5])


# ---- voxel_hash.h -------------------------------------------------------------------------------------------------------------------

def test_voxel_keys_round_trip_on_host_and_device():
    B = 1 << 20
    edge = [-B, -B + 1, -2, -1, 0, 1, 2, B - 2, B - 1]
    k = np.array(list(itertools.product(edge, repeat=3)), I32)
    k = np.repeat(k, 8, axis=0)
    d = np.tile(np.arange(8, dtype=U32), len(k) // 8)
    step = np.stack([d & 1, (d >> 1) & 1, d >> 2], axis=1).astype(I32)
    ok = ((k + step) < B).all(axis=1)                            # voxel_neighbour: no field at its last value along a set bit of d
    k, d, step = pad256(k[ok]), pad256(d[ok]), pad256(step[ok])

    def key(c):
        c = c.astype(np.int64) + B
        return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    want = np.concatenate([key(k)[:, None], key(k + step)[:, None], k.astype(np.int64)], axis=1)
    assert np.array_equal(H.call("voxel_key", np.zeros((len(k), 5), np.int64), k, d), want)
    assert np.array_equal(H.host_voxel_key(k, d), want)
    assert len(np.unique(want[:, 0])) == len(np.unique(k, axis=0))


def test_map_hash_is_the_splitmix64_finaliser():
    rng = np.random.default_rng(27)
    k = rng.integers(0, 2 ** 63, 1024, dtype=U64) * U64(2) + rng.integers(0, 2, 1024).astype(U64)
    k[:4] = [0, 1, M64, 0x9E3779B97F4A7C15]
    got = H.call("map_hash", np.zeros(len(k), U32), k)
    assert np.array_equal(got, np.array([W.map_hash(int(x)) for x in k], U32))


def _run_waves():
    rng = np.random.default_rng(28)
    w = [np.full(64, 42), np.arange(64) + 100]                                    # all equal; all distinct
    w.append(np.r_[np.full(63, 1), 2])                                            # a run ending at lane 62, a one-lane run at lane 63
    w.append(np.r_[np.full(40, 1), np.full(24, 2)])                               # a run ending at lane 63
    w.append(np.r_[7, np.full(63, 1)])                                            # a one-lane run at lane 0
    w.append(np.r_[np.full(62, 1), 2, 3])                                         # one-lane runs at lanes 62 and 63
    w.append(np.r_[np.full(31, 1), np.full(2, 2), np.full(31, 1)])                # the same key again in a later run
    for _ in range(9):
        w.append(np.repeat(rng.integers(0, 2 ** 40, 64), rng.integers(1, 9, 64))[:64])
    hi = np.concatenate(w).astype(U64)
    return pad256((hi << U64(32)) | (hi >> U64(3)))                               # keys that differ in either half


def test_voxel_runs_and_run_heads():
    key = _run_waves()
    got = H.call("voxel_runs", np.zeros((len(key), 3), I32), key)
    want = np.zeros_like(got)
    for w in range(0, len(key), 64):
        k = key[w:w + 64]
        head = np.r_[True, k[1:] != k[:-1]]
        heads = np.nonzero(head)[0]
        for lane in range(64):
            nxt = heads[heads > lane]
            want[w + lane] = (head[lane], (nxt[0] if len(nxt) else 64) - lane, heads[heads <= lane][-1])
    assert np.array_equal(got, want)


def test_voxel_list_position_hands_out_a_permutation():
    rng = np.random.default_rng(29)
    n = 4096
    take = (rng.random(n) < 0.4).astype(I32)
    take[0:64] = 0                                                # no lane takes: false, and no atomic
    take[64:128] = 1                                              # all lanes
    for i, lane in enumerate((0, 31, 32, 63)):                    # one lane
        take[128 + 64 * i:192 + 64 * i] = 0
        take[128 + 64 * i + lane] = 1
    take[-64:] = 0
    at, ret, total = H.list_position(take)
    tw = take.reshape(-1, 64)
    assert np.array_equal(ret, np.repeat(tw.any(axis=1), 64).astype(I32))
    assert total == take.sum()
    assert np.array_equal(np.sort(at[take == 1]), np.arange(total, dtype=U64))
    for w in np.nonzero(tw.any(axis=1))[0]:                       # inside a wave: consecutive, in lane order
        a = at[w * 64:(w + 1) * 64]
        lower = np.cumsum(tw[w]) - tw[w]
        assert np.array_equal(a - a.min(), lower.astype(U64)), w


EMPTY = U64(M64)


def _keys_by_home(rng, count, want_home, mask=1023):
    out = []
    while len(out) < count:
        k = int(rng.integers(0, 2 ** 62))
        if want_home(W.map_hash(k) & mask):
            out.append(k)
    return out


def test_voxel_probe_and_find_on_a_raw_table():
    """4096 threads insert 700 distinct keys, heavily repeated, into 1024 slots: every key lands once, the probe's slot is where
    voxel_find finds it, and the chains of the keys whose home is in the table's last slots go on at slot 0."""
    rng = np.random.default_rng(30)
    keys = _keys_by_home(rng, 60, lambda h: h >= 1004) + _keys_by_home(rng, 640, lambda h: True)
    keys = np.array(sorted(set(keys)), U64)
    assert len(keys) == 700
    use = np.ascontiguousarray(np.concatenate([keys, keys[rng.integers(0, 700, 4096 - 700)]])[rng.permutation(4096)])
    table = np.full(1024, EMPTY, U64)
    slot, claimed, ret = H.voxel_probe(table, use)
    assert (ret == 1).all()
    assert np.array_equal(np.sort(table[table != EMPTY]), keys)              # every key present exactly once
    assert np.array_equal(table[slot], use)
    assert claimed.sum() == 700 and len(np.unique(use[claimed == 1])) == 700   # one claim per key
    home = np.array([W.map_hash(int(k)) & 1023 for k in use], U32)
    assert (slot < home).any()                                                # chains cross the table's end
    fslot, _, fret = H.voxel_probe(table, use, find=True)
    assert (fret == 1).all() and np.array_equal(fslot, slot)
    absent = np.array(_keys_by_home(rng, 256, lambda h: True), U64)
    assert not np.isin(absent, keys).any()
    _, _, fret = H.voxel_probe(table, absent, find=True)
    assert (fret == 0).all()


def test_voxel_probe_and_find_on_a_full_table():
    rng = np.random.default_rng(31)
    table = rng.permutation(np.arange(1, 1025, dtype=U64) * U64(0x10001))    # no empty slot
    before = table.copy()
    fresh = np.arange(5000, 5128, dtype=U64) * U64(0x10001)
    use = np.ascontiguousarray(np.concatenate([before[:128], fresh]))
    slot, claimed, ret = H.voxel_probe(table, use)
    assert np.array_equal(table, before) and (claimed == 0).all()
    assert (ret[:128] == 1).all() and np.array_equal(table[slot[:128]], use[:128])
    assert (ret[128:] == 0).all()                                            # every slot visited once, then false: no hang
    fslot, _, fret = H.voxel_probe(table, use, find=True)
    assert (fret[:128] == 1).all() and np.array_equal(fslot[:128], slot[:128]) and (fret[128:] == 0).all()


# ---- solver_dev.h -------------------------------------------------------------------------------------------------------------------

EPS = np.finfo(F64).eps


def _jacobian_systems(oracle, rng, count, twin):
    """Normal equations J'J, J'r of 3-point reprojection Jacobians (the oracle's compute_J); twin: two of the points identical."""
    param = Param.kitti00()
    out = []
    for _ in range(count):
        X = np.stack([rng.uniform(-10, 10, 3), rng.uniform(-2, 2, 3), rng.uniform(4, 60, 3)])
        if twin:
            X[:, 1] = X[:, 0]
        obs = np.stack([param.f * X[0] / X[2] + param.cu, param.f * X[1] / X[2] + param.cv, param.f * (X[0] - param.base) / X[2] + param.cu,
                        param.f * X[1] / X[2] + param.cv]) + rng.normal(0, 0.5, (4, 3))
        if twin:
            obs[:, 1] = obs[:, 0]
        J, _, res = oracle.compute_J(X, obs, rng.normal(0, 0.02, 6), param, np.arange(3))
        out.append((J.T @ J, J.T @ res))
    return out


def _pivot_column(rng, step, column):
    """A 6 x 6 system whose elimination reaches `step` untouched (identity rows above it) and finds `column` there, from the diagonal
    down; the rest random."""
    A = np.eye(6)
    A[step:, step:] = rng.uniform(-2, 2, (6 - step, 6 - step))
    A[step:, step] = column
    return A, rng.uniform(-1, 1, 6)


def _swap_steps(A):
    """The steps at which the LU swaps rows (pivot choice restated; only used to see that the inputs cover every step)."""
    A = A.copy()
    steps = []
    for i in range(6):
        k = i
        for j in range(i + 1, 6):
            if abs(A[j, i]) > abs(A[k, i]):
                k = j
        if abs(A[k, i]) < EPS:
            break
        if k != i:
            A[[i, k]] = A[[k, i]]
            steps.append(i)
        for j in range(i + 1, 6):
            A[j, i + 1:] += (A[j, i] * (-1 / A[i, i])) * A[i, i + 1:]
    return steps


def test_lu_solve6_is_the_oracles_lu_bit_for_bit(oracle):
    """The device's lu_solve6 and oracle.lu_solve6 on the same 6 x 6 systems: the verdict always, and with verdict 1 all six solution
    doubles, bit for bit (a NaN as a NaN: its sign and payload are no property of IEEE arithmetic).  This is the comparison behind the open finding on near-degenerate triples: with the same
    matrix on both sides the two LUs agree, singular verdicts at the threshold included, so that difference is in the matrices
    (sincos, accumulation order), not here."""
    rng = np.random.default_rng(32)
    sys_ = _jacobian_systems(oracle, rng, 150, False) + _jacobian_systems(oracle, rng, 60, True)
    for _ in range(40):                                           # rank 5 by construction: the last pivot is rounding
        J = rng.normal(0, 1, (12, 5)) @ rng.normal(0, 1, (5, 6))
        sys_.append((J.T @ J, J.T @ rng.normal(0, 1, 12)))
    general = [(rng.uniform(-2, 2, (6, 6)), rng.uniform(-1, 1, 6)) for _ in range(120)]
    swapped = set(s for A, _ in general for s in _swap_steps(A))
    assert swapped == {0, 1, 2, 3, 4}                             # a row swap at each of the five steps
    sys_ += general
    up, dn = np.nextafter(EPS, 1.0), np.nextafter(EPS, 0.0)
    for step in range(6):
        m = 6 - step
        for piv in (EPS, up, dn, -EPS, -dn):                      # a pivot at DBL_EPSILON and one ulp on either side, at each step
            col = np.full(m, piv * 0.5)
            col[int(rng.integers(m))] = piv
            sys_.append(_pivot_column(rng, step, col))
        if m >= 3:                                                # equal magnitudes: the first strict maximum wins
            for col in ([2.0, -2.0, 2.0], [1.0, -2.0, 2.0], [-1.0, 1.0, -1.0], [0.5, 2.0, -2.0]):
                c = np.r_[col, rng.uniform(-0.4, 0.4, m - 3)]
                sys_.append(_pivot_column(rng, step, c))
    for pos in ((0, 0), (3, 1), (5, 5), (2, 4)):                  # a NaN entry
        A, b = rng.uniform(-2, 2, (6, 6)), rng.uniform(-1, 1, 6)
        A[pos] = np.nan
        sys_.append((A, b))
    A = pad256(np.array([a for a, _ in sys_]).reshape(-1, 36))
    b = pad256(np.array([v for _, v in sys_]))
    got = H.call("lu_solve6", np.zeros((len(A), 7)), A, b)
    verdicts = []
    for i in range(len(sys_)):
        ok, x = oracle.lu_solve6(A[i].reshape(6, 6), b[i])
        verdicts.append(ok)
        assert int(got[i, 6]) == ok, (i, ok, A[i])
        if ok:
            nan = np.isnan(x)
            assert np.array_equal(np.isnan(got[i, :6]), nan), i
            same_bits(got[i, :6][~nan], x[~nan], "system %d" % i)
    assert 0 in verdicts and 1 in verdicts
    twins = verdicts[150:250]
    print("near-singular systems (twin points, rank 5): %d of %d called singular, on both sides alike" % (twins.count(0), len(twins)))


def test_sample3_and_its_generator_on_device_host_and_oracle(oracle):
    rng = np.random.default_rng(33)
    s = rng.integers(0, 2 ** 63, 1024, dtype=U64) * U64(2) + U64(1)
    s[:3] = [0, M64, 0x9E3779B97F4A7C15]
    got = H.call("splitmix64", np.zeros((len(s), 2), U64), s)
    assert np.array_equal(got, H.host_splitmix64(s))
    assert np.array_equal(got, np.array([W.splitmix64(int(x)) for x in s], U64))
    a, b = s, np.ascontiguousarray(np.roll(s, 7) >> rng.integers(0, 64, len(s)).astype(U64))
    got = H.call("mulhi64", np.zeros(len(a), U64), a, b)
    assert np.array_equal(got, H.host_mulhi64(a, b))
    assert np.array_equal(got, np.array([(int(x) * int(y)) >> 64 for x, y in zip(a, b)], U64))
    for N in (0, 1, 2, 3, 4, 5, 7, 1000, 2 ** 31 - 1):
        for seed, frame in ((3, 12), (2 ** 64 - 1, 2 ** 40)):
            iters = 256
            arg = np.ascontiguousarray(np.stack([np.full(iters, seed, U64), np.full(iters, frame, U64), np.arange(iters, dtype=U64)], axis=1))
            Ns = np.full(iters, N, I32)
            got = H.call("sample3", np.full((iters, 3), -1, I32), arg, Ns)
            assert np.array_equal(got, H.host_sample3(arg, Ns)), N
            assert np.array_equal(got, oracle.ransac_samples(seed, frame, iters, N)), N
            if N >= 3:
                assert (got[:, 0] < got[:, 1]).all() and (got[:, 1] < got[:, 2]).all() and got.min() >= 0 and got.max() < N
            else:
                assert (got == 0).all()


def test_up6_is_the_upper_triangle_row_by_row():
    p, q = np.triu_indices(6)
    p, q = pad256(p.astype(I32)), pad256(q.astype(I32))
    got = H.call("up6", np.zeros(len(p), I32), p, q)
    assert np.array_equal(got[:21], np.arange(21))


def test_write_cov6():
    """cov = sigma2 L^-T L^-1 from the lower-triangular L^-1, each entry summed over k = q .. 5 in that order, then scaled."""
    rng = np.random.default_rng(34)
    nb = 5
    Li = np.tril(rng.normal(0, 1, (nb, 6, 6)) * 10.0 ** rng.uniform(-3, 3, (nb, 6, 6)))
    sigma2 = rng.uniform(0.1, 4.0, nb)
    got = H.write_cov6(Li.reshape(nb, 36), sigma2).reshape(nb, 6, 6)
    for blk in range(nb):
        for p in range(6):
            for q in range(p, 6):
                v = 0.0
                for k in range(q, 6):
                    v += Li[blk, k, p] * Li[blk, k, q]
                v *= sigma2[blk]
                assert got[blk, p, q] == v and got[blk, q, p] == v, (blk, p, q)
        assert np.allclose(got[blk], sigma2[blk] * Li[blk].T @ Li[blk], rtol=1e-12, atol=0)
