"""The inputs of tests/test_gpu_subpixel_edges.py, checked on the restatement alone (tests/subpixel_cases.py,
tests/subpixel_ref.py): every case reaches the branch of subpixel_refine_kernel it claims to reach, so no GPU test passes
by never visiting one.  Runs without a device."""
import numpy as np
import pytest

import subpixel_cases as SC
import subpixel_ref as S
from test_subpixel_cpu import _sobel_windows


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def test_classifier_hand_cases():
    assert SC.is_fast([7, 7], 16, 15) and not SC.is_fast([6, 7], 16, 15) and not SC.is_fast([8, 7], 16, 15)
    assert not SC.is_fast([7, 6], 16, 15) and not SC.is_fast([7, 8], 16, 15)          # qy + 7 < rows - 1
    assert not SC.is_fast([7, 7], 15, 15) and not SC.is_fast([7, 7], 16, 14)
    assert SC.is_fast([7, 8], 17, 15) and not SC.is_fast([7, 9], 17, 15)
    assert not SC.is_fast([2.0 ** 31, 7], 16, 15) and not SC.is_fast([7, -3e38], 16, 15)
    cc = lambda *a: SC.cost_class(*a).item()                                          # noqa: E731
    assert cc(7, 7, 7) == SC.FLAT and cc(0, 0, 0) == SC.FLAT
    assert cc(3, 5, 9) == SC.NOT_MIN and cc(9, 5, 3) == SC.NOT_MIN and cc(4, 5, 4) == SC.NOT_MIN
    assert cc(5, 5, 9) == SC.PLATEAU and cc(9, 5, 5) == SC.PLATEAU
    assert cc(9, 4, 9) == SC.INTERIOR and cc(10, 4, 6) == SC.INTERIOR
    # the classes are the branches of the offset: only an interior minimum or a plateau moves the point
    rng = np.random.default_rng(0)
    s = rng.integers(0, 6, (4000, 3))
    c = SC.cost_class(s[:, 0], s[:, 1], s[:, 2])
    off = S.parabola_offset(s[:, 0], s[:, 1], s[:, 2])
    assert set(c.tolist()) == set(SC.CLASSES)
    assert (off[(c == SC.FLAT) | (c == SC.NOT_MIN)] == 0).all()
    assert (np.abs(off[c == SC.PLATEAU]) == 0.5).all() and (np.abs(off[c == SC.INTERIOR]) < 0.5).all()


def test_every_position_shapes_cover_the_residues():
    assert {c & 3 for r, c in SC.EVERY_SHAPES if r <= 17} == {0, 1, 2, 3}
    wide = [(r, c) for r, c in SC.EVERY_SHAPES if r > 17]
    assert {c & 3 for _, c in wide} == {0, 1, 2, 3}
    for r, c in wide:                                   # several fast columns and rows
        assert c - 14 >= 20 and r - 15 >= 5


@pytest.mark.parametrize("shape", SC.EVERY_SHAPES, ids=_ids)
@pytest.mark.parametrize("kind", ["random", "smooth"])
def test_every_position_reaches_both_staging_paths(shape, kind):
    rows, cols = shape
    imgL, imgR, kp1, kp2, match = SC.every_position(rows, cols, kind)
    assert imgL.shape == imgR.shape == shape and imgL.dtype == np.uint8 and not np.array_equal(imgL, imgR)
    q, p = SC.row_q(kp2, match), SC.row_p(kp1, match)
    fast = SC.is_fast(q, rows, cols)
    assert fast.any() and (~fast).any()
    if shape == (16, 15):
        assert fast.sum() == 1 and tuple(q[fast][0]) == (7, 7)
    assert fast.sum() == (cols - 14) * (rows - 15)
    # every integer position of the image and of the ring of 8, on the right and on the left
    want = {(x, y) for x in range(-8, cols + 8) for y in range(-8, rows + 8)}
    assert {tuple(v) for v in q.tolist()} == want and {tuple(v) for v in p.tolist()} == want
    assert len(q) == len(want)
    # both sides of the predicate in x (on a row that passes in y) and in y (on a column that passes in x); the last fast
    # row rows - 9 is the one whose region stops one image row short of the buffer's end
    yok = (q[:, 1] >= 7) & (q[:, 1] + 7 < rows - 1)
    xok = (q[:, 0] >= 7) & (q[:, 0] + 7 < cols)
    for x, f in ((6, False), (7, True), (cols - 8, True), (cols - 7, False)):
        sel = yok & (q[:, 0] == x)
        assert sel.any() and (fast[sel] == f).all(), (x, f)
    for y, f in ((6, False), (7, True), (rows - 9, True), (rows - 8, False)):
        sel = xok & (q[:, 1] == y)
        assert sel.any() and (fast[sel] == f).all(), (y, f)


@pytest.mark.parametrize("cols", [16, 17, 18, 19])
def test_costs_agree_with_the_independent_extractor(oracle, cols):
    """One shape per cols & 3: the restatement the GPU test compares against (the oracle's extractor) and the whole-image
    Sobel of tests/test_subpixel_cpu.py give the same five costs at every position, border ring included."""
    rows = 16
    imgL, imgR, kp1, kp2, match = SC.every_position(rows, cols, "random")
    Sx, Sy = S.costs(oracle, imgL, imgR, kp1, kp2, match)
    p, q = SC.row_p(kp1, match).astype(int), SC.row_q(kp2, match).astype(int)
    wl = _sobel_windows(imgL, p)
    for c, d in enumerate((-1, 0, 1)):
        assert np.array_equal(Sx[:, c], np.abs(wl - _sobel_windows(imgR, q + [d, 0])).sum(1))
        assert np.array_equal(Sy[:, c], np.abs(wl - _sobel_windows(imgR, q + [0, d])).sum(1))
    assert len(set(SC.cost_class(Sx[:, 0], Sx[:, 1], Sx[:, 2]).tolist())) >= 3


def test_rounding_values():
    rows, cols = SC.ROUND_SHAPE
    imgL, imgR, kp1, kp2, match = SC.rounding()
    f32 = np.float32
    for kp in (kp1, kp2):
        xs, ys = set(kp[:, 0].tolist()), set(kp[:, 1].tolist())
        assert {-0.5, 0.5, 1.5, 2.5, 3.5, 5.5, 6.5, 7.5, cols - 8.5, cols - 7.5, cols - 6.5, cols - 0.5, cols + 0.5} <= xs
        assert {-0.5, 0.5, 1.5, 2.5, 3.5, 5.5, 6.5, 7.5, rows - 9.5, rows - 8.5, rows - 7.5, rows - 0.5, rows + 0.5} <= ys
        for h in (-0.5, 0.5, 2.5, 3.5, 6.5, cols - 7.5):
            for to in (-np.inf, np.inf):
                assert float(np.nextafter(f32(h), f32(to))) in xs, (h, to)
        for h in (-0.5, 0.5, 2.5, 3.5, 6.5, rows - 8.5):
            for to in (-np.inf, np.inf):
                assert float(np.nextafter(f32(h), f32(to))) in ys, (h, to)
    # half to even, not half away: the halves on both parities, and the neighbours fall to either side
    r = lambda v: float(np.rint(f32(v)))                                              # noqa: E731
    assert (r(2.5), r(3.5), r(0.5), r(6.5), r(7.5)) == (2, 4, 0, 6, 8) and np.signbit(np.rint(f32(-0.5)))
    assert r(np.nextafter(f32(6.5), f32(np.inf))) == 7 and r(np.nextafter(f32(7.5), f32(-np.inf))) == 7
    # the halves round onto both sides of the fast predicate, in x and in y
    q = SC.row_q(kp2, match)
    fast = SC.is_fast(q, rows, cols)
    frac = kp2[match[:, 1]] - np.floor(kp2[match[:, 1]])
    hx, hy = frac[:, 0] == 0.5, frac[:, 1] == 0.5
    for x in (6, 8, cols - 8, cols - 6):
        assert (hx & (q[:, 0] == x)).any(), x
    for y in (6, 8, rows - 10, rows - 8):
        assert (hy & (q[:, 1] == y)).any(), y
    assert (hx & fast).any() and (hx & ~fast).any() and (hy & fast).any() and (hy & ~fast).any()
    assert ((q[:, 0] < 0) | (q[:, 0] >= cols)).any() and ((q[:, 1] < 0) | (q[:, 1] >= rows)).any()


def test_a_zero_is_positive_in_both_modes(oracle):
    """q is an integer in the header's definition, so a right keypoint in [-0.5, -0] gives +0 in mode 1 as (float)q.y and
    in mode 2 as (float)((double)q.y + off): the restatement never returns the -0 that rint leaves behind."""
    imgL, imgR, kp1, kp2, match = SC.rounding()
    assert np.signbit(np.rint(kp2[match[:, 1]]))[SC.row_q(kp2, match) == 0].any()
    for mode in (1, 2):
        uv = S.refine(oracle, imgL, imgR, kp1, kp2, match, mode)
        assert (uv == 0).any() and not np.signbit(uv[uv == 0]).any()


@pytest.fixture(scope="module")
def tie_set(oracle):
    return SC.ties(oracle)


def test_tie_set_holds_every_class(oracle, tie_set):
    count = {ax: {c: 0 for c in SC.CLASSES} for ax in "xy"}
    names = {c: set() for c in SC.CLASSES}
    for name, case, cx, cy in tie_set:
        imgL, imgR, kp1, kp2, match = case
        assert imgL.shape == SC.TIE_SHAPE and len(match) == len(cx) == len(cy) and len(match) <= 1500
        Sx, Sy = S.costs(oracle, *case)
        assert np.array_equal(SC.cost_class(Sx[:, 0], Sx[:, 1], Sx[:, 2]), cx)
        assert np.array_equal(SC.cost_class(Sy[:, 0], Sy[:, 1], Sy[:, 2]), cy)
        for ax, cls_of, C in (("x", cx, Sx), ("y", cy, Sy)):
            off = S.parabola_offset(C[:, 0], C[:, 1], C[:, 2])
            assert (np.abs(off[cls_of == SC.PLATEAU]) == 0.5).all()       # exactly one half
            assert (off[(cls_of == SC.FLAT) | (cls_of == SC.NOT_MIN)] == 0).all()
            for c in SC.CLASSES:
                k = int((cls_of == c).sum())
                count[ax][c] += k
                if k:
                    names[c].add(name)
    for ax in "xy":
        for c in SC.CLASSES:
            assert count[ax][c] >= SC.TIE_MIN, (ax, c, count)
    # the constructed candidates suffice: the plateaus come from the ramps, the two-pixel stripes and the two-valued images
    assert names[SC.PLATEAU] & {"ramp-x", "stripes-x2", "two-valued-0"}


@pytest.mark.parametrize("which", ["right", "left", "both"])
def test_far_away_expectation(oracle, which):
    ext = oracle.extract_descriptors
    for mode in (1, 2):
        # where the oracle's extractor is defined the analytic expectation is the restatement
        for case in (SC.far_away(which, SC.FAR_SMALL), SC.far_away(which, SC.FAR_HUGE, limit=SC.FAR_OK)):
            assert np.array_equal(SC.analytic_refine(ext, *case, mode).view(np.uint32), S.refine(oracle, *case, mode).view(np.uint32))
        imgL, imgR, kp1, kp2, match = case = SC.far_away(which, SC.FAR_HUGE)
        rows, cols = imgL.shape
        far = kp2 if which != "left" else kp1
        big = np.abs(far).max(1)
        assert big.min() >= 2.0 ** 31 and big.max() == np.float32(3.0e38) and np.isfinite(far).all()
        assert (far.max(1) >= 2.0 ** 31).any() and (far.min(1) <= -2.0 ** 31).any()
        got = SC.analytic_refine(ext, *case, mode)
        q, p = SC.row_q(kp2, match), SC.row_p(kp1, match)
        if which != "left":        # five equal costs: the rounded keypoint itself, in both modes
            assert SC.window_outside(q, rows, cols).all()
            assert np.array_equal(got.view(np.uint32), (np.rint(kp2[match[:, 1]]) + np.float32(0)).view(np.uint32))
        else:                      # W_L = 0: the parabola through sum |W_R|
            assert SC.window_outside(p, rows, cols).all() and not SC.window_outside(q, rows, cols).any()
            assert SC.is_fast(q, rows, cols).any() and not SC.is_fast(q, rows, cols).all()
            s = [np.abs(ext(imgR, (q + [d, 0]).astype(np.float32))).sum(1).astype(np.int64) for d in (-1, 0, 1)]
            assert np.array_equal(got[:, 0], (q[:, 0] + S.parabola_offset(*s)).astype(np.float32))
            assert (got[:, 0] != q[:, 0]).any()
    # the analytic form is the restatement on ordinary rows too
    case = SC.every_position(17, 18, "random")
    assert np.array_equal(SC.analytic_refine(ext, *case, 2), S.refine(oracle, *case, 2))


def test_list_lengths_cover_the_row_bookkeeping():
    assert {n % 4 for n in SC.LENGTHS} == {0, 1, 2, 3}                 # 1, 2, 3 and 4 active DPP rows in the last wave
    assert {255, 256, 257} <= set(SC.LENGTHS) and max(SC.LENGTHS) > 2 * 256   # one sweep of 16 blocks x 16 rows, +-1; a third pass
    rows, cols = SC.LENGTH_SHAPE
    for n in SC.LENGTHS:
        for kind in SC.LENGTH_KINDS:
            imgL, imgR, kp1, kp2, match = SC.list_length(n, kind)
            n1, n2 = len(kp1), len(kp2)
            assert len(match) == n and imgL.shape == (rows, cols)
            assert match[:, 0].min() >= 0 and match[:, 0].max() < n1 and match[:, 1].min() >= 0 and match[:, 1].max() < n2
            if kind == "larger":
                assert n1 > n and n2 > n
            elif kind == "smaller":
                assert (n1 < n and n2 < n) or n == 1                   # the scratch blocks are sized by n
            else:
                assert n1 == 1 and (match[:, 0] == 0).all()
            shared = np.bincount(match[:, 1]).max()
            assert shared >= (n + 2) // 3
            if n >= 15:
                f = SC.is_fast(SC.row_q(kp2, match), rows, cols)
                assert f.any() and (~f).any()


@pytest.mark.parametrize("shape", SC.DEGENERATE_SHAPES, ids=_ids)
def test_degenerate_shapes(oracle, shape):
    rows, cols = shape
    imgL, imgR, kp1, kp2, match = case = SC.degenerate(rows, cols)
    q = SC.row_q(kp2, match)
    assert not SC.is_fast(q, rows, cols).any() and len(q) == (rows + 16) * (cols + 16)
    uv = S.refine(oracle, *case, 2)
    if min(rows, cols) == 1:       # no Sobel centre inside the image: every window is zero, nothing moves
        assert np.array_equal(uv.view(np.uint32), (q + 0.0).astype(np.float32).view(np.uint32))
    elif shape != (2, 2):
        assert (uv != q).any()


@pytest.mark.parametrize("cols", SC.BATCH_WIDTHS)
def test_batch_cases(oracle, cols):
    rows = SC.BATCH_ROWS
    for small in (True, False):
        first, second = SC.batch_case(cols, small)
        cap = first["cap"]
        assert second["cap"] == cap and first["images"].shape[2:] == (rows, cols) and len(first["n"]) >= 4
        assert (cap == 5) if small else (cap % 16 != 0 and cap > 256)
        assert max(first["n"].max(), second["n"].max()) <= cap
        e1, e2 = SC.batch_expected(oracle, first, 2), SC.batch_expected(oracle, second, 2)
        l1, l2 = [len(m) for m, _ in e1], [len(m) for m, _ in e2]
        n = first["n"]
        assert ((n == 0).any(1) & (n > 0).any(1)).any()                # a frame with no keypoints on one side
        assert any(k == 0 and n[t].min() > 0 for t, k in enumerate(l1))   # a list that comes out empty from two full sides
        assert len({k for k in l1 if k}) >= 2                          # clearly different list lengths
        if not small:
            assert len({k for k in l1 if k}) >= 3 and max(l1) >= 3 * min(k for k in l1 if k)
            assert max(l1) > 256 and min(k for k in l1 if k) < 64      # past one sweep of the grid, and under one block's share
        f, s = SC.batch_fast_counts(first, [m for m, _ in e1])
        assert (f >= 1 and s >= 1) if small else (f >= 8 and s >= 8)
        # the second upload: shorter lists, one of them empty where the first had rows, rows where the first had none
        assert sum(l2) < sum(l1) and sum(a > b for a, b in zip(l1, l2)) >= 2
        assert any(a > 0 and b == 0 for a, b in zip(l1, l2)) and any(a == 0 and b > 0 for a, b in zip(l1, l2))
        for (m, uv2), (_, uv1) in zip(e1, SC.batch_expected(oracle, first, 1)):     # the modes share uR' and differ in vR'
            assert np.array_equal(uv1[:, 0], uv2[:, 0]) and (small or len(m) == 0 or (uv1[:, 1] != uv2[:, 1]).any())
