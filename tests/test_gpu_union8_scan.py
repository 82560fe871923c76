"""The union kernels' scan (phase 1) and match_union8_kernel's rescue byte at the places where the scan's two 32-target
steps meet: one tile (at most 64 queries), radius 80, integer coordinates, the two descriptor families of
tests/matcher_cases.py.  Every case goes through a Batch against oracle.match_desc: match list, scored-pair counter and
m_out, on matcher variants 6 (match_union8_kernel) and 3 (match_union_kernel), with the planes' shift forced to the
families' 3 and left to the data.

Where a case needs a keypoint at a given place of the scan, the place is proven here, without the device (`staged`): the
target image's y range is [0, 8192], so the tile's 64 y buckets are 128 rows high (the bucket scale 2^-7 is exact), the staged
window is in bucket order, an iteration of the scan covers staged positions 64 i .. 64 i + 63 (step a the first 32), and a
keypoint that is alone in its bucket sits at the number of keypoints in the buckets below.  Inside a bucket the order is
not defined; no claim rests on it."""
import functools

import numpy as np
import pytest

import libviso_amd
import matcher_cases as MC
from libviso_amd.abi import MatchParams, Param

pytestmark = pytest.mark.gpu

QX, R = MC.QX, MC.RADIUS
YTOP, BH = 8192, 128          # target y range and the height of a y bucket
YB = 8 * BH                   # a bucket border: y < YB is bucket 7, y >= YB bucket 8


def staged(kp2):
    """(y bucket of every target, targets in lower buckets, targets in its own bucket): the staged position of a target is
    below + (its place among `same`)."""
    y = np.asarray(kp2)[:, 1]
    assert y.min() == 0 and y.max() == YTOP
    b = np.clip((y / BH).astype(int), 0, 63)
    below = np.array([(b < v).sum() for v in b])
    same = np.array([(b == v).sum() for v in b])
    return b, below, same


def _case(name, q, tg, family, sums=None, twins=(), K=250, second=1, check=None):
    """tg[0] is target 0 (outside every radius unless it is the only one).  clear family: MC._clear plants one best per query;
    flat family: sums = the targets' SADs.  twins = (a, b): target b gets a's descriptor (an exact tie wherever both are
    candidates)."""
    kp1, kp2 = np.asarray(q, np.float32), np.asarray(tg, np.float32)
    mp = MC._params(K, second)
    D = MC.l1(kp1, kp2)
    M = D <= np.float32(R)
    assert len(kp1) <= MC.QPB and MC.window(kp1, kp2, R).all(), "one tile whose window is the whole image"
    if family == "clear":
        d1, d2, _ = MC._clear(np.random.default_rng(MC._seed("scan", name)), M, np.zeros(len(kp1), bool), None, D, K)
    else:
        d1, d2 = MC._flat(M, np.asarray(sums, int))
    for a, b in [twins] if twins else []:
        d2[b] = d2[a]
    c = MC.Case(name, kp1, kp2, d1, d2, mp, dict(M=M))
    if check:
        check(c)
    return c


def _far(n, x0=QX - 70, y0=YB + 400):
    """n fillers inside the window and far above every query in y (never in radius)"""
    return [(x0 + i % 41, y0 + 3 * i) for i in range(n)]


def _low(n):
    """n fillers in the buckets below bucket 7 (y < 896): staged in front of everything near y = YB"""
    return [(QX - 40 + i % 81, 1 + (5 * i) % (7 * BH - 1)) for i in range(n)]


ANCH = [(QX, 0), (QX, YTOP)]     # target 0 and the y range's other end


def _steps_case(name, where, twins=False):
    """One query 60 rows above a bucket border, so that its diamond touches buckets 7, 8 and 9: member A alone in bucket 7
    with where[0] keypoints below it, fillers (out of radius) in bucket 8, member B alone in bucket 9 at staged position
    where[1]."""
    pa, pb = where
    q = [(QX, YB + 60)]
    A, B = (QX + 3, YB - 10), (QX - 4, YB + BH + 2)
    low = _low(pa - 1)           # ANCH[0] is below as well
    mid = [(QX - 75 + i % 5, YB + i % 20) for i in range(pb - pa - 1)]   # bucket 8, |dx| + |dy| >= 115
    tg = [ANCH[0]] + low + [A] + mid + [B, ANCH[1]]
    iA, iB = 1 + len(low), 1 + len(low) + 1 + len(mid)

    def check(c):
        b, below, same = staged(c.kp2)
        assert c.claims["M"][0, iA] and c.claims["M"][0, iB] and c.claims["M"].sum() == 2
        assert (b[iA], below[iA], same[iA]) == (7, pa, 1) and (b[iB], below[iB], same[iB]) == (9, pb, 1)
    # a tie is only visible in the result without the ratio test (with it the query is rejected either way)
    return _case(name, q, tg, "clear", twins=(iA, iB) if twins else (), second=0 if twins else 1, check=check)


def _one_step_case(name, pos):
    """one member, alone in its bucket, at staged position pos"""
    q = [(QX, YB)]
    tg = [ANCH[0]] + _low(pos - 1) + [(QX + 2, YB + 7), ANCH[1]]

    def check(c):
        _, below, same = staged(c.kp2)
        assert c.claims["M"].sum() == 1 and below[pos] == pos and same[pos] == 1
    return _case(name, q, tg, "clear", check=check)


def _halves_case():
    """eight queries 10 rows apart (y rank k = query k of the round); one target in radius of queries 0..3 only, one of
    queries 4..7 only, one of all eight"""
    q = [(QX, YB + 10 * k) for k in range(8)]
    tg = [ANCH[0], (QX + 5, YB - 40), (QX + 5, YB + 70 + 40), (QX - 3, YB + 35), ANCH[1]] + _far(20, y0=YB + 900)

    def check(c):
        M = c.claims["M"]
        assert M[:, 1].tolist() == [True] * 4 + [False] * 4 and M[:, 2].tolist() == [False] * 4 + [True] * 4 and M[:, 3].all()
    return _case("halves", q, tg, "clear", check=check)


def _window_case(W):
    """a window of W keypoints in all; 8 queries around one cluster"""
    if W == 1:
        return _case("W1", [(QX, YB)], [(QX + 3, YB + 4)], "clear")
    q = [(QX, YB + 10 * k) for k in range(8)]
    nm = min(20, W - 2)
    mem = [(QX - 10 + i % 21, YB + 30 + i // 21 * 5 + i % 3) for i in range(nm)]
    tg = [ANCH[0]] + mem + _low(W - 2 - nm) + [ANCH[1]]
    assert len(tg) == W
    return _case(f"W{W}", q, tg, "clear")


def _queries_case(nq):
    """nq queries 100 rows apart (several rounds and waves; dead slots past the tile's last query), three members each, the
    neighbours' out of reach"""
    q = [(QX + (k % 5), 1000 + 100 * k) for k in range(nq)]
    mem = [(QX + dx, 1000 + 100 * k + dy) for k in range(nq) for dx, dy in ((-12, 3), (7, -9), (20, 11))]
    return _case(f"q{nq}", q, [ANCH[0]] + mem + [ANCH[1]], "clear")


def _tail_case(extra):
    """W = 512 + extra: 12 members at the window's start (small x), fillers, 20 members at its end (large x): the window
    is in column-bucket order, so the last 20 positions are the second group's — on both sides of position 512 for
    extra < 20, all in the tail beyond"""
    W = MC.KPCAP + extra
    q = [(QX, YB + 10 * k) for k in range(8)]
    lowm = [(QX - 40 + i, YB + 33 + i % 4) for i in range(12)]
    highm = [(QX + 25 + i % 10, YB + 35 + i // 10) for i in range(20)]
    fil = [(QX - 25 + i % 46, YB + 300 + 3 * i) for i in range(W - 2 - 32)]
    tg = [fil[0], (QX - 25, 0)] + fil[1:] + lowm + highm + [ANCH[1]]   # target 0: a filler; then the y range's lower end
    assert len(tg) == W

    def check(c):
        b, _, _ = MC.buckets(c.kp2)
        hi = np.arange(W - 21, W - 1)
        assert c.claims["M"][:, hi].all() and (b[hi].min() > np.delete(b, hi).max())   # the window's last 20 positions
        lo_ = np.arange(W - 33, W - 21)
        assert c.claims["M"][:, lo_].all() and (b[lo_].max() < np.delete(b, lo_).min())
    return _case(f"tail+{extra}", q, tg, "clear", check=check)


def _rescue_case(nu):
    """flat family: every plane byte equal, so every query with three or more members needs the rescue.  Eight queries that
    share nu members (from nu = 8 on, two of them belong to the first / the last four queries only: their cells of the
    other queries are non-members whose byte reads 255)"""
    q = [(QX, YB + 10 * k) for k in range(8)]
    part = [(QX + 5, YB - 40), (QX + 5, YB + 110)] if nu >= 8 else []
    shared = [(QX - 8 + i % 17, YB + 33 + i // 17 * 3) for i in range(nu - len(part))]
    tg = [ANCH[0]] + shared + part + [ANCH[1]] + _far(10, y0=YB + 900)
    sums = [5] + [1] + [10 + i for i in range(nu - 1)] + [5] * 11

    def check(c):
        M = c.claims["M"]
        assert M.any(0).sum() == nu and (M.sum(1) >= 3).all() and nu <= MC.S8ROWS
    return _case(f"rescue-nu{nu}", q, tg, "flat", sums=sums, check=check)


@functools.lru_cache(None)
def cases():
    out = [_steps_case("a-only", (5, 6))]                        # both members in step a
    out.append(_steps_case("b-only", (40, 41)))                  # both in step b
    out.append(_steps_case("a-and-b", (10, 50)))                 # one in each
    out.append(_steps_case("31|32", (31, 32)))
    out.append(_steps_case("63|64", (63, 64)))
    out.append(_one_step_case("below-range", 100))               # the scan starts at 64, 36 positions below the member's bucket
    out.append(_steps_case("tie-31|32", (31, 32), twins=True))   # equal SAD8 and SAD, one in each step: largest-key rule
    out.append(_steps_case("tie-63|64", (63, 64), twins=True))   # ... one in each of two iterations
    out.append(_halves_case())
    out += [_window_case(W) for W in (1, 63, 64, 65, 127, 128, 129)]
    out += [_queries_case(n) for n in (1, 7, 9, 63, 64)]
    out += [_tail_case(e) for e in (1, 31, 32, 33, 63, 64, 65)]
    out += [_rescue_case(nu) for nu in (3, 8, 17)]
    return out


@functools.lru_cache(None)
def wanted():
    from oracle import pyoracle
    return [pyoracle.match_desc(*c.args(), return_scored=True) for c in cases()]


def test_the_cases_sit_where_they_claim():
    assert len({c.name for c in cases()}) == len(cases())
    for c, (m, sc) in zip(cases(), wanted()):
        assert sc == int(c.claims["M"].sum()) or c.name == "W1", c.name    # (W1: target 0 is in radius, src/viso.cpp:693)
    byname = dict(zip((c.name for c in cases()), wanted()))
    assert len(byname["halves"][0]) >= 1 and all(len(byname[f"rescue-nu{n}"][0]) >= 1 for n in (3, 8, 17))


@pytest.mark.parametrize("shift", [MC.R8_SHIFT, -1], ids=["shift3", "shift-free"])
@pytest.mark.parametrize("variant", [6, 3])
def test_scan_cases_against_the_oracle(viso, variant, shift):
    assert variant in libviso_amd.MATCHER_VARIANTS
    F = MC.rectified_F()
    ctx = libviso_amd.Context(0)
    try:
        libviso_amd.set_matcher_variant(variant, ctx)
        libviso_amd.set_row8_shift(shift, ctx)
        for c, (want, wsc) in zip(cases(), wanted()):
            kp1, kp2, d1, d2, mp = c.args()
            n1, n2 = len(kp1), len(kp2)
            cap = max(n1, n2)
            kp = np.zeros((2, 2, cap, 2), np.float32)
            desc = np.zeros((2, 2, cap, MC.DLEN), np.float32)
            n = np.zeros((2, 2), np.int32)
            kp[0, 0, :n2], desc[0, 0, :n2], kp[1, 0, :n1], desc[1, 0, :n1] = kp2, d2, kp1, d1
            n[0, 0], n[1, 0] = n2, n1
            b = libviso_amd.Batch(ctx, 2, cap)
            try:
                b.upload(kp, desc, n)
                b.set_params(MatchParams.stereo(F), mp, Param.default(), seed=1)
                b.run_matcher()
                got = b.matches(1, 1)
                sc, mo = b.counters()
                assert np.array_equal(got, want), (c.name, variant, shift, len(got), len(want))
                assert int(sc[1, 1]) == wsc and int(mo[1, 1]) == len(want), (c.name, variant, shift, int(sc[1, 1]), wsc, int(mo[1, 1]))
                if shift >= 0 and variant == 6:
                    assert b.row8_shift() == shift
            finally:
                b.close()
    finally:
        ctx.close()
