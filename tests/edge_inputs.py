"""Inputs that sit on the edges of two kernels, shared by the GPU tests and by the CPU test of the inputs themselves.

1. extract_pack_kernel (csrc/extract.hip).  Nothing reads the packed rows back, so the matcher is made to: a match row is
   (query, train, dist) and dist is the SAD of the two packed rows.  Every image of a case carries the SAME keypoint
   positions, distinct points of the half-pixel grid, and both matchers run with radius 0.25 (L1): the only candidate of a
   keypoint is its counterpart at the identical position, so one wrong descriptor element anywhere shows up in dist.  The
   images are independent random bytes, so errors cannot cancel.

   The reference's neighbour walk stops at target index 0 (match_desc, src/viso.cpp:692-693: `row[j] > 0`), so whatever
   sits at index 0 of a train list is never matched.  Index 0 of every image is therefore a sentinel that is not part of
   the probe: an image with `n` probe keypoints holds n + 1 keypoints, and each of the three match lists has exactly n
   rows (queries 1..n).  The probe counts are chosen so that the images' totals cover a single keypoint, last waves of
   1, 2 and 3 keypoints, full waves and more than one workgroup.

2. circle_table_kernel<LDS> behind viso_match_circle (csrc/circle.hip): lists the way match_desc emits them (unique query
   keys in match11, match_lr_prev and match22), consistent circles planted on every third row of match_lr, the other rows
   random, with the largest key chosen so that the table size lands where the kernel changes path.
"""
import numpy as np

from libviso_amd.abi import MatchParams, Param
from libviso_amd import hostmath, synth

# ---------------------------------------------------------------------------------------------------- extract_pack rows
NF = 3
FAR = float(2 ** 20)            # both forms of every comparison in the kernel are well defined there
RADIUS = 0.25                   # L1; distinct half-pixel grid points are >= 0.5 apart
SHAPES = [(40, 72), (13, 13), (12, 30), (30, 12), (7, 5), (2, 2), (1, 9)]
COUNTS = (1, 3, 5, 64, 65, 257)             # probe keypoints per image (the image holds one more: the sentinel)
# on the first shape also the counts whose TOTALS are 1, 3, 5, 64 and 257 keypoints per image
EXTRA_COUNTS = (0, 2, 4, 63, 256)
CAP_PADS = (0, 1, 3)                        # cap = total + pad: cap % VISO_EXT_KPW != 0 occurs for every count
RAGGED_COUNTS = np.array([[6, 3], [2, 5], [4, 7]], np.int32)   # totals 7 4 / 3 6 / 5 8: last waves of 3, 0, 3, 2, 1, 0
ROW8_SHIFTS = (-1, 0, 1, 2, 3)
V8 = 6


def position_set(rows, cols):
    """Distinct half-pixel grid points on and around every edge the kernel tests, in a fixed order."""
    pts = []

    def add(x, y):
        pts.append((float(x), float(y)))

    for x in (0, cols - 1):
        for y in (0, rows - 1):
            add(x, y)                                        # the four corner pixels
    xm, ym = cols // 2, rows // 2
    for d in range(8):                                       # distance 0..7 from each edge, alone and two edges at once
        if d < cols:
            add(d, (3 * d + 1) % rows); add(cols - 1 - d, (5 * d + 2) % rows)
        if d < rows:
            add((3 * d + 1) % cols, d); add((5 * d + 2) % cols, rows - 1 - d)
        if d < min(rows, cols):
            add(d, d); add(cols - 1 - d, rows - 1 - d); add(d, rows - 1 - d); add(cols - 1 - d, d)
    for d in range(1, 9):                                    # 1..8 px outside on every side, and past the corners
        add(-d, (2 * d) % rows); add(cols - 1 + d, (2 * d + 1) % rows)
        add((2 * d) % cols, -d); add((2 * d + 1) % cols, rows - 1 + d)
        add(-d, -d); add(cols - 1 + d, rows - 1 + d); add(-d, rows - 1 + d); add(cols - 1 + d, -d)
    # .5 coordinates: rintf rounds ties to even, so 4.5 -> 4, 5.5 -> 6, 6.5 -> 6, and the same around len - 6 and the edges
    hx = [-5.5, -0.5, 0.5, 4.5, 5.5, 6.5, cols - 7.5, cols - 6.5, cols - 5.5, cols - 1.5, cols - 0.5, cols + 4.5]
    hy = [-5.5, -0.5, 0.5, 4.5, 5.5, 6.5, rows - 7.5, rows - 6.5, rows - 5.5, rows - 1.5, rows - 0.5, rows + 4.5]
    for i, x in enumerate(hx):
        add(x, ym); add(x, hy[i]); add(x, hy[(i + 5) % len(hy)])
    for y in hy:
        add(xm, y)
    for dx, dy in ((0, 0), (1, -1), (-2, 1), (3, 2)):        # a few interior points
        add(min(max(xm + dx, 0), cols - 1), min(max(ym + dy, 0), rows - 1))
    add(FAR, FAR); add(-FAR, -FAR)                           # two far points
    return list(dict.fromkeys(pts))


def positions(rows, cols, n, seed):
    """n distinct positions: the whole set (repeated with fresh half-pixel offsets while it is smaller than n), shuffled."""
    base = position_set(rows, cols)
    have = dict.fromkeys(base)
    offs = [(0.5 * a, 0.5 * b) for s in range(1, 12) for a in range(s + 1) for b in range(s + 1) if max(a, b) == s]
    for ox, oy in offs:
        if len(have) >= n:
            break
        for x, y in base:
            have.setdefault((x + ox, y + oy))
    pts = np.array(list(have), np.float64)
    assert len(pts) >= n
    rng = np.random.default_rng(seed)
    if n >= len(base):                 # every position of the set is in, the rest drawn from the repeats
        idx = np.concatenate([np.arange(len(base)), len(base) + rng.permutation(len(pts) - len(base))[:n - len(base)]])
    else:
        idx = rng.permutation(len(base))[:n]
    out = pts[rng.permutation(idx)].astype(np.float32)
    assert np.array_equal(out.astype(np.float64) * 2, np.rint(out.astype(np.float64) * 2))   # exact in float32
    assert len({tuple(p) for p in out.tolist()}) == n
    return out


def sentinel(rows, cols):
    """Index 0 of every image: a position of its own (never matched: the reference's walk stops at target index 0)."""
    return np.array([cols + 100.5, rows + 100.5], np.float32)


def match_params():
    F = hostmath.F_from_P(synth.KITTI_P1, synth.KITTI_P2)
    st, tm = MatchParams.stereo(F), MatchParams.temporal()
    st.radius = RADIUS
    tm.radius = RADIUS
    tm.enforce_2nd_best = 0
    assert st.enforce_2nd_best == 0
    return st, tm


def extract_case(shape, counts, pad, kind="random"):
    """images [NF][2][rows][cols] uint8, kp [NF][2][cap][2], n [NF][2] (totals: probes + the sentinel), cap.
    counts: probe keypoints per image, an int or an [NF][2] array (ragged).  kind: "random" or "columns" (every column
    0 or 255: Sobel-x reaches +-1020, the full range of the planes)."""
    rows, cols = shape
    counts = np.broadcast_to(np.asarray(counts, np.int32), (NF, 2))
    nmax = int(counts.max())
    seed = 1000003 * rows + 1009 * cols + 17 * nmax + (7 if kind == "columns" else 0) + int(counts.min())
    rng = np.random.default_rng(seed)
    if kind == "columns":
        images = np.broadcast_to((rng.integers(0, 2, (NF, 2, 1, cols)) * 255).astype(np.uint8), (NF, 2, rows, cols)).copy()
    else:
        images = rng.integers(0, 256, (NF, 2, rows, cols)).astype(np.uint8)   # six independent images
    pos = np.concatenate([sentinel(rows, cols)[None], positions(rows, cols, nmax, seed + 1)])
    n = (counts + 1).astype(np.int32)
    cap = nmax + 1 + pad
    kp = np.full((NF, 2, cap, 2), FAR, np.float32)             # slots past n hold (2^20, 2^20)
    for t in range(NF):
        for side in range(2):
            kp[t, side, :n[t, side]] = pos[:n[t, side]]
    return dict(images=images, kp=kp, n=n, cap=cap, counts=counts.copy(), shape=shape)


def problems():
    """(which, t, query image, train image) of the batch's match lists; an image is (t, side)."""
    out = []
    for t in range(NF):
        out.append((0, t, (t, 0), (t, 1)))
        if t > 0:
            out.append((1, t, (t, 0), (t - 1, 0)))
            out.append((2, t, (t, 1), (t - 1, 1)))
    return out


def extract_expected(oracle, case):
    """The oracle's descriptors [NF][2][cap][121], and per problem (which, t) -> (match list, scored pairs)."""
    kp, n, cap = case["kp"], case["n"], case["cap"]
    desc = np.zeros((NF, 2, cap, 121), np.float32)
    for t in range(NF):
        for side in range(2):
            k = n[t, side]
            desc[t, side, :k] = oracle.extract_descriptors(case["images"][t, side], kp[t, side, :k])
    st, tm = match_params()
    lists = {}
    for which, t, q, g in problems():
        nq, ng = n[q], n[g]
        lists[which, t] = oracle.match_desc(kp[q][:nq], kp[g][:ng], desc[q][:nq], desc[g][:ng], st if which == 0 else tm,
                                            return_scored=True)
    return desc, lists


def check_probe_is_full(case, lists):
    """The condition on the oracle alone: no probe keypoint escapes.  Every list holds exactly the probe keypoints that
    both images of its problem have (all n of them when the case is not ragged), each matched to its counterpart."""
    n = case["n"]
    for which, t, q, g in problems():
        m, _ = lists[which, t]
        both = int(min(n[q], n[g])) - 1                        # probe keypoints 1..both exist in both images
        assert len(m) == both, (case["shape"], which, t, len(m), both)
        assert np.array_equal(np.sort(m[:, 0]), 1 + np.arange(both)), (case["shape"], which, t)
        assert np.array_equal(m[:, 0], m[:, 1]), (case["shape"], which, t)
    if case["counts"].min() == case["counts"].max():
        k = int(case["counts"][0, 0])
        assert all(len(lists[w, t][0]) == k for w, t, _, _ in problems())


def matcher_configs(variants):
    """(variant, row8 shift) pairs: every variant of the build, and for match_union8_kernel every plane shift."""
    return [(v, s) for v in variants for s in (ROW8_SHIFTS if v == V8 else (-1,))]


def default_param():
    return Param.kitti00()


# ------------------------------------------------------------------------------------------- per-call circle join
CIRCT_LDS_TABN = 6144          # csrc/circle.hip: tables of up to this many keys live in LDS, larger ones in global scratch
CIRC_TAB_MAX = 1 << 20         # keys from here on (and negative ones) send the call to the literal loops
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def _unique(rng, K, n, avoid=None, must=None):
    """n distinct keys of [0, K), none of `avoid`, `must` among them."""
    if K <= 4 * (n + (len(avoid) if avoid is not None else 0)) + 16:
        pool = np.setdiff1d(np.arange(K), avoid if avoid is not None else [])
        if must is not None:
            pool = pool[pool != must]
        keys = rng.permutation(pool)[:n - (must is not None)]
    else:                                                      # a large key space: draw, drop repeats, refill
        taken = set(int(a) for a in avoid) if avoid is not None else set()
        if must is not None:
            taken.add(int(must))
        keys = []
        while len(keys) < n - (must is not None):
            for k in rng.integers(0, K, n).tolist():
                if k not in taken and len(keys) < n - (must is not None):
                    taken.add(k); keys.append(k)
        keys = np.array(keys, np.int64)
    if must is not None:
        keys = rng.permutation(np.concatenate([keys, [must]]))
    assert len(keys) == n and len(set(keys.tolist())) == n
    return keys.astype(np.int32)


def circle_lists(seed, n_lr, tabn, n_keyed=None):
    """(lr, lr_prev, m11, m22), each [rows][3] int32, keys in [0, tabn) with tabn - 1 present in lr_prev (so the call's
    table size is exactly tabn).  Circles are planted the way test_match_circle_general plants them, on every third row
    of lr: lr (i, a), m11 (i, b), lr_prev (b, c), m22 (a, c); the keyed lists' rows are then shuffled."""
    rng = np.random.default_rng(seed)
    K = int(tabn)
    n_keyed = n_lr if n_keyed is None else n_keyed
    assert 1 <= n_lr <= K and 1 <= n_keyed <= K
    lr = np.stack([_unique(rng, K, n_lr), _unique(rng, K, n_lr), rng.integers(0, 999, n_lr)], 1).astype(np.int32)
    lrp = np.stack([_unique(rng, K, n_keyed, must=K - 1), rng.integers(0, K, n_keyed), rng.integers(0, 999, n_keyed)], 1).astype(np.int32)
    planted = np.arange(0, min(n_lr, n_keyed), 3)
    other = np.setdiff1d(np.arange(n_keyed), planted)
    m11 = np.zeros((n_keyed, 3), np.int32)
    m22 = np.zeros((n_keyed, 3), np.int32)
    m11[planted, 0], m11[planted, 1] = lr[planted, 0], lrp[planted, 0]
    m22[planted, 0], m22[planted, 1] = lr[planted, 1], lrp[planted, 1]
    m11[other, 0] = _unique(rng, K, len(other), avoid=lr[planted, 0])
    m22[other, 0] = _unique(rng, K, len(other), avoid=lr[planted, 1])
    m11[other, 1] = rng.integers(0, K, len(other))
    m22[other, 1] = rng.integers(0, K, len(other))
    m11[:, 2] = rng.integers(0, 999, n_keyed)
    m22[:, 2] = rng.integers(0, 999, n_keyed)
    lrp, m11, m22 = (a[rng.permutation(n_keyed)] for a in (lrp, m11, m22))
    for a in (lrp, m11, m22):
        assert len(np.unique(a[:, 0])) == len(a)
    assert max(lrp[:, 0].max(), m11[:, 0].max(), m22[:, 0].max()) == K - 1
    return [np.ascontiguousarray(a) for a in (lr, lrp, m11, m22)]


KEYED = {"lr_prev": 1, "m11": 2, "m22": 3}     # position of the keyed lists in circle_lists' result


def _free_row(lists, which):
    """A row of keyed list `which` that no planted circle of lr uses (so changing it costs no joined row)."""
    lr, a = lists[0], lists[KEYED[which]]
    used = set(lr[:, 0].tolist()) | set(lr[:, 1].tolist())
    for r in range(len(a) - 1, -1, -1):
        if int(a[r, 0]) not in used:
            return r
    return len(a) - 1


def circle_cases():
    """name -> dict(lists, table=bool: the call stays on the tables, lds=bool or None, caps=None or 'truncate')."""
    cases = {}

    def put(name, lists, table=True, **kw):
        cases[name] = dict(lists=lists, table=table, **kw)

    # table size: tabn = largest key + 1; 1707 is the first size past 40 KB of dynamic LDS, 6145 the first global one
    for tabn in (1, 1706, 1707, 6143, 6144, 6145, 20000, CIRC_TAB_MAX):
        put(f"tabn-{tabn}", circle_lists(100 + tabn % 997, min(300, tabn), tabn))
    # one key that forces the literal loops, lists of at most 300 rows
    for which in KEYED:
        for key in (CIRC_TAB_MAX, -1):
            lists = circle_lists(200 + KEYED[which], 300, 400)
            lists[KEYED[which]][_free_row(lists, which), 0] = key
            put(f"literal-{which}-key{key}", lists, table=False)
    # rows: one pass, the pass boundary, two and three passes of the 1024-thread loop, on both table paths
    for tabn in (CIRCT_LDS_TABN, 20000):
        for n_lr in (1, 1023, 1024, 1025, 3000):
            put(f"rows-{n_lr}-tabn-{tabn}", circle_lists(300 + n_lr, n_lr, tabn, n_keyed=max(n_lr, 64)))
    # truncation, two passes, both table paths (the caps come from the oracle's row count)
    for tabn in (CIRCT_LDS_TABN, 20000):
        put(f"truncate-tabn-{tabn}", circle_lists(400 + tabn % 7, 1500, tabn), truncate=True)
    # keys outside the tables in lr (either column) and values outside them in m11
    for tabn in (500, 20000):
        lists = circle_lists(500 + tabn % 11, 300, tabn)
        lr, m11 = lists[0], lists[2]
        bad = [-1, -5, tabn, tabn + 7, CIRC_TAB_MAX, 2 ** 30, I32_MAX, I32_MIN]
        for i, v in enumerate(bad):
            lr[1 + 3 * i, 0] = v                              # rows 1, 4, ...: not planted
            lr[2 + 3 * i, 1] = v                              # rows 2, 5, ...: not planted
        lr[30, 0], lr[33, 1] = -1, tabn                       # two planted rows as well
        for i, v in enumerate(bad):
            m11[7 * i + 3, 1] = v                             # wherever the shuffle put them, planted ones included
        put(f"outside-tabn-{tabn}", lists)
    # a duplicate key in the LAST row of one keyed list only: found by the last thread of the build, after which the
    # whole call has to take the literal loops
    for which in KEYED:
        for name, n_lr, tabn in (("lds", 300, 500), ("global", 300, 20000), ("two-pass", 1025, 2000)):
            lists = circle_lists(600 + 10 * KEYED[which] + n_lr % 7, n_lr, tabn, n_keyed=300)
            a = lists[KEYED[which]]
            a[-1, 0] = a[0, 0]
            put(f"late-dup-{which}-{name}", lists, table=False)
    # empty lists
    for which in KEYED:
        lists = circle_lists(700 + KEYED[which], 300, 400)
        lists[KEYED[which]] = np.zeros((0, 3), np.int32)
        put(f"empty-{which}", lists, table=None)
    lists = circle_lists(710, 300, 400)
    put("empty-all-keyed", [lists[0]] + [np.zeros((0, 3), np.int32)] * 3, table=None)
    put("empty-lr", [np.zeros((0, 3), np.int32)] + circle_lists(711, 300, 400)[1:], table=None)
    return cases


def check_circle_joins(name, case, n_out):
    """The condition on the oracle alone: a case that stays on the tables joins at least a quarter of its rows."""
    if case["table"]:
        n_lr = len(case["lists"][0])
        assert n_out >= max(1, n_lr // 4), (name, n_out, n_lr)
    elif case["table"] is False:
        assert n_out > 0, name
