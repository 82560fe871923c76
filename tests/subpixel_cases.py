"""Inputs that sit on the edges of subpixel_refine_kernel (csrc/subpixel.hip), shared by tests/test_gpu_subpixel_edges.py
and by the CPU test of the inputs themselves (tests/test_subpixel_cases_cpu.py), plus a classifier of the kernel's branches.

The kernel stages the right region of a stereo row on one of two paths (`fast`: five aligned dwords per region row, the
byte shift of row rr re-derived as (s0 + rr * (cols & 3)) & 3; else byte gathers with reflect-101), builds its output on
rintf(kp2) while a clamped integer carries the address, takes one of four branches in subpix_off per axis, and shares a wave
among four stereo rows.  Every generator below aims at one of these; each returns (imgL, imgR, kp1, kp2, match).

No GPU and no library import at module level: the generators that need descriptor costs take the `oracle` fixture.
"""
import numpy as np

FAST_MARGIN = 7                 # the 15 x 15 region of q reaches 7 pixels to every side
RING = 8                        # keypoints up to this far outside the image
FAR_OK = float(2 ** 20)         # the oracle's extractor (lrintf to int) is defined up to here and beyond; the cases stop here
FLAT, NOT_MIN, PLATEAU, INTERIOR = "flat", "not_min", "plateau", "interior"
CLASSES = (FLAT, NOT_MIN, PLATEAU, INTERIOR)

EVERY_SHAPES = [(r, c) for r in (16, 17) for c in (15, 16, 17, 18, 19)] + [(24, c) for c in (40, 41, 42, 43)]
LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)
LENGTH_KINDS = ("larger", "smaller", "one_left")
LENGTH_SHAPE = (40, 64)
DEGENERATE_SHAPES = [(1, 1), (1, 50), (50, 1), (2, 2), (3, 3), (15, 15), (16, 14)]
TIE_SHAPE = (24, 40)
TIE_MIN = 8                     # rows of every class the tie set must hold, per axis
ROUND_SHAPE = (24, 40)
BATCH_ROWS = 40
BATCH_WIDTHS = (97, 98, 99, 100)
BATCH_DISP = 3


# ------------------------------------------------------------------------------------------------------ the classifier
def is_fast(q, rows, cols):
    """The kernel's staging predicate on q = np.rint(kp2[i2]) ([..., 2], x then y)."""
    q = np.asarray(q, np.float64)
    qx, qy = q[..., 0], q[..., 1]
    return (qx >= FAST_MARGIN) & (qx + FAST_MARGIN < cols) & (qy >= FAST_MARGIN) & (qy + FAST_MARGIN < rows - 1)


def row_q(kp2, match):
    """q of every row of `match`: np.rint of the right keypoint, float64."""
    kp2 = np.asarray(kp2, np.float32).reshape(-1, 2)
    match = np.asarray(match, np.int32).reshape(-1, 3)
    return np.rint(kp2[match[:, 1]]).astype(np.float64)


def row_p(kp1, match):
    kp1 = np.asarray(kp1, np.float32).reshape(-1, 2)
    match = np.asarray(match, np.int32).reshape(-1, 3)
    return np.rint(kp1[match[:, 0]]).astype(np.float64)


def cost_class(sm, s0, sp):
    """The branch of subpix_off a cost triple takes: an array of FLAT / NOT_MIN / PLATEAU / INTERIOR."""
    sm, s0, sp = (np.asarray(a, np.int64) for a in (sm, s0, sp))
    den = sm + sp - 2 * s0
    is_min = (s0 <= sm) & (s0 <= sp)
    out = np.full(np.broadcast(sm, s0, sp).shape, INTERIOR, dtype=object)
    out[is_min & (den > 0) & ((s0 == sm) | (s0 == sp))] = PLATEAU
    out[is_min & (den <= 0)] = FLAT
    out[~is_min] = NOT_MIN
    return out


def _ident_match(n, perm=None, seed=0):
    rng = np.random.default_rng(seed)
    left = np.arange(n) if perm is None else perm
    return np.stack([left, np.arange(n), rng.integers(0, 9999, n)], 1).astype(np.int32)


def _images(rows, cols, kind, seed):
    from libviso_amd import synth
    rng = np.random.default_rng(seed)
    if kind == "smooth":
        return synth.make_images(seed, rows, cols), synth.make_images(seed + 1, rows, cols)
    return rng.integers(0, 256, (rows, cols), dtype=np.uint8), rng.integers(0, 256, (rows, cols), dtype=np.uint8)


def grid_positions(rows, cols, ring=RING):
    """Every integer position of the image and of a ring around it, row by row."""
    ys, xs = np.meshgrid(np.arange(-ring, rows + ring), np.arange(-ring, cols + ring), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)


# --------------------------------------------------------------------------------------------------- every position
def every_position(rows, cols, kind="random", seed=0):
    """kp2 = every integer position of the image plus a ring of 8 pixels; row i pairs right keypoint i with the left
    keypoint at a shuffled position of the same set, so the left positions cover the border ring too."""
    seed = 7919 * rows + 31 * cols + seed + (1 if kind == "smooth" else 0)
    imgL, imgR = _images(rows, cols, kind, seed)
    kp2 = grid_positions(rows, cols)
    rng = np.random.default_rng(seed + 5)
    kp1 = kp2[rng.permutation(len(kp2))].copy()
    return imgL, imgR, kp1, kp2, _ident_match(len(kp2), seed=seed)


# --------------------------------------------------------------------------------------------------------- rounding
def half_values(length):
    """Coordinates around the halves: k - 0.5 and k + 0.5 for every integer k near 0, near both sides of the fast predicate
    and near `length` (even and odd k alike), and the float32 neighbours of each half on either side."""
    ks = sorted(set(range(-2, 10)) | set(range(length - 10, length + 2)))
    vals = []
    for k in ks:
        for h in (np.float32(k - 0.5), np.float32(k + 0.5)):
            vals += [h, np.nextafter(h, np.float32(-np.inf)), np.nextafter(h, np.float32(np.inf))]
    return np.array(sorted(set(float(v) for v in vals)), np.float32)


def rounding(rows=ROUND_SHAPE[0], cols=ROUND_SHAPE[1], seed=0):
    """Both keypoints carry fractional parts of exactly +-0.5 (and the floats next to them) in x, in y and in both."""
    imgL, imgR = _images(rows, cols, "random", 991 + seed)
    vx, vy = half_values(cols), half_values(rows)
    ym, xm = float(rows // 2), float(cols // 2)            # a fast row / column: the other coordinate decides alone
    assert is_fast([xm, ym], rows, cols)
    pts = [(x, ym) for x in vx] + [(xm, y) for y in vy] + [(vx[i % len(vx)], vy[(7 * i) % len(vy)]) for i in range(max(len(vx), len(vy)))]
    pts += [(x, vy[(3 * i + 1) % len(vy)]) for i, x in enumerate(vx)]
    kp2 = np.array(pts, np.float32)
    rng = np.random.default_rng(17 + seed)
    kp1 = kp2[rng.permutation(len(kp2))].copy()
    return imgL, imgR, kp1, kp2, _ident_match(len(kp2), seed=seed)


# --------------------------------------------------------------------------------------------------------- far away
FAR_SMALL = (100.0, 5000.0, 65536.0, FAR_OK)
FAR_HUGE = (2.0 ** 31, 2.0 ** 31 + 256.0, 4.0e9, 2.0 ** 40, 1.0e19, 1.0e30, 3.0e38)


def _far_points(mags, rows, cols, rng):
    """Points with one or both coordinates at +-mag, the other inside the image."""
    pts = []
    for m in mags:
        for s in (-1.0, 1.0):
            pts.append((s * m, float(rng.integers(0, rows))))
            pts.append((float(rng.integers(0, cols)), s * m))
            pts.append((s * m, -s * m))
            pts.append((s * m, s * m))
    return np.array(pts, np.float32)


def far_away(which, mags=FAR_SMALL, rows=24, cols=40, seed=0, limit=None):
    """which = "right", "left" or "both": the side whose keypoints lie at +-mag; the other side's are inside the image,
    some of them fast.  mags = FAR_SMALL stays where the oracle's extractor is defined, FAR_HUGE goes beyond an int.
    limit: the same rows with every far coordinate moved to +-limit."""
    rng = np.random.default_rng(4441 + seed)
    imgL, imgR = _images(rows, cols, "random", 313 + seed)
    far = _far_points(mags, rows, cols, rng)
    if limit is not None:
        far = np.clip(far, -limit, limit).astype(np.float32)
    n = len(far)
    near = np.stack([rng.integers(0, cols, n), rng.integers(0, rows, n)], 1).astype(np.float32)
    near[::3] = [cols // 2, rows // 2]                       # a fast position
    kp1 = far if which in ("left", "both") else near
    kp2 = far[::-1].copy() if which == "both" else (far if which == "right" else near)
    return imgL, imgR, kp1, kp2, _ident_match(n, seed=seed)


def window_outside(p, rows, cols):
    """True where the 11 x 11 window at the integer point p has no Sobel centre inside the image (it is all zero)."""
    p = np.asarray(p, np.float64)
    return (p[..., 0] + 5 < 1) | (p[..., 0] - 5 > cols - 1) | (p[..., 1] + 5 < 1) | (p[..., 1] - 5 > rows - 1)


def analytic_refine(extract, imgL, imgR, kp1, kp2, match, mode):
    """The header's definition with the windows that lie wholly outside the image written down as zeros instead of
    extracted: defined for every finite keypoint.  extract(img, pts) -> [n][121] is only called with points whose window
    touches the image.  Returns [n][2] float32."""
    import subpixel_ref as S
    rows, cols = imgL.shape
    p, q = row_p(kp1, match), row_q(kp2, match)
    n = len(p)

    def windows(img, pts):
        w = np.zeros((n, 121), np.int64)
        inside = ~window_outside(pts, rows, cols)
        if inside.any():
            w[inside] = np.asarray(extract(img, pts[inside].astype(np.float32)), np.float64).astype(np.int64)
        return w

    wl = windows(imgL, p)
    Sx, Sy = np.empty((n, 3), np.int64), np.empty((n, 3), np.int64)
    for c, d in enumerate((-1, 0, 1)):
        Sx[:, c] = np.abs(wl - windows(imgR, q + [d, 0])).sum(1)
        Sy[:, c] = np.abs(wl - windows(imgR, q + [0, d])).sum(1)
    uv = np.empty((n, 2), np.float32)
    uv[:, 0] = (q[:, 0] + S.parabola_offset(Sx[:, 0], Sx[:, 1], Sx[:, 2])).astype(np.float32)
    oy = S.parabola_offset(Sy[:, 0], Sy[:, 1], Sy[:, 2]) if mode == 2 else 0.0
    uv[:, 1] = (q[:, 1] + oy).astype(np.float32)
    return uv


# ------------------------------------------------------------------------------------------------------------- ties
def tie_candidates(rows=TIE_SHAPE[0], cols=TIE_SHAPE[1]):
    """name -> (imgL, imgR): images built so that descriptor costs collide."""
    rng = np.random.default_rng(271)
    y, x = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)     # noqa: E731
    tex = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    out = {}
    out["constant"] = (u8(np.full((rows, cols), 90)), u8(np.full((rows, cols), 200)))
    out["constant-along-x"] = (u8(np.broadcast_to(rng.integers(0, 256, (rows, 1)), (rows, cols))),
                               u8(np.broadcast_to(rng.integers(0, 256, (rows, 1)), (rows, cols))))
    out["ramp-x"] = (u8(3 * x + 10), u8(3 * x + 10))
    out["ramp-x-vs-steeper"] = (u8(3 * x + 10), u8(5 * x))
    out["same"] = (tex, tex.copy())
    out["shift-x"] = (tex, np.roll(tex, 1, axis=1))
    out["shift-y"] = (tex, np.roll(tex, 1, axis=0))
    out["checkerboard"] = (u8(255 * ((x + y) & 1)), u8(255 * ((x + y + 1) & 1)))
    out["stripes-x"] = (u8(255 * (x & 1)), u8(255 * (x & 1)))
    out["stripes-y"] = (u8(255 * (y & 1)), u8(255 * ((y + 1) & 1)))
    out["stripes-x2"] = (u8(255 * ((x >> 1) & 1)), u8(255 * (((x + 1) >> 1) & 1)))
    for s in range(3):
        r = np.random.default_rng(600 + s)
        a = (r.integers(0, 2, (rows, cols)) * 255).astype(np.uint8)
        b = a.copy()
        flip = r.random((rows, cols)) < 0.1
        b[flip] = 255 - b[flip]
        out[f"two-valued-{s}"] = (a, b)
    return out


def ties(oracle, per_class=12):
    """[(name, (imgL, imgR, kp1, kp2, match), classes_x, classes_y)]: from every candidate pair, up to per_class rows of
    each class in x and up to per_class of each in y, found among q = every position of the image and a ring of 2 pixels,
    p = q, q + (1, 0) and q + (0, 1)."""
    import subpixel_ref as S
    out = []
    for name, (imgL, imgR) in tie_candidates().items():
        rows, cols = imgL.shape
        kp2 = grid_positions(rows, cols, ring=2)
        m = len(kp2)
        kp1 = np.concatenate([kp2, kp2 + np.float32([1, 0]), kp2 + np.float32([0, 1])])
        match = np.concatenate([_ident_match(m, np.arange(m) + k * m, seed=k) for k in range(3)])
        Sx, Sy = S.costs(oracle, imgL, imgR, kp1, kp2, match)
        cx, cy = cost_class(Sx[:, 0], Sx[:, 1], Sx[:, 2]), cost_class(Sy[:, 0], Sy[:, 1], Sy[:, 2])
        rng = np.random.default_rng(len(name))
        keep = set()
        for cls_of in (cx, cy):
            for c in CLASSES:
                idx = np.flatnonzero(cls_of == c)
                keep |= set(rng.permutation(idx)[:per_class].tolist())
        keep = np.array(sorted(keep), np.int64)
        out.append((name, (imgL, imgR, kp1, kp2, np.ascontiguousarray(match[keep])), cx[keep], cy[keep]))
    return out


# ----------------------------------------------------------------------------------------------------- list lengths
def list_length(n, kind, seed=0):
    """A list of n rows on one 40 x 64 pair.  kind "larger": both keypoint sets hold more than n; "smaller": both hold
    fewer (the scratch blocks are then sized by n); "one_left": a single left keypoint.  A third of the rows share one
    right keypoint."""
    rows, cols = LENGTH_SHAPE
    imgL, imgR = _images(rows, cols, "random", 77)
    n1, n2 = {"larger": (n + 7, n + 3), "smaller": (max(1, n // 2), max(1, n // 3)), "one_left": (1, n + 2)}[kind]
    rng = np.random.default_rng(1000 * n + len(kind) + seed)
    kp1 = np.stack([rng.integers(-RING, cols + RING, n1), rng.integers(-RING, rows + RING, n1)], 1).astype(np.float32)
    kp2 = np.stack([rng.integers(-RING, cols + RING, n2), rng.integers(-RING, rows + RING, n2)], 1).astype(np.float32)
    kp2[n2 // 2] = [cols // 2, rows // 2]                        # the shared one is a fast position
    match = np.stack([rng.integers(0, n1, n), rng.integers(0, n2, n), rng.integers(0, 9999, n)], 1).astype(np.int32)
    match[::3, 1] = n2 // 2
    return imgL, imgR, kp1, kp2, match


# ---------------------------------------------------------------------------------------------- degenerate geometry
def degenerate(rows, cols, seed=0):
    return every_position(rows, cols, "random", seed + 100)


# ------------------------------------------------------------------------------------------------------ batch frames
def _lattice(rows, cols):
    """Right-image positions: the border, both sides of the fast predicate in x and in y, and a coarse grid between."""
    xs = sorted({0, 1, 5, 6, 7, 8, 9, cols - 10, cols - 9, cols - 8, cols - 7, cols - 6, cols - 2, cols - 1} | set(range(14, cols - 10, 5)))
    ys = sorted({0, 6, 7, 8, 14, 20, 26, rows - 10, rows - 9, rows - 8, rows - 7, rows - 1})
    return [(x, y) for y in ys for x in xs]


def _frame(rng, rows, cols, right_pts, related=True, right_dy=0, left_n=None, right_n=None):
    """One stereo frame: imgR a random texture, imgL the same texture BATCH_DISP pixels to the right (or an unrelated one);
    left keypoint = right keypoint + (BATCH_DISP, 0); right_dy moves the right keypoints off the left ones' rows."""
    imgR = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    imgL = np.roll(imgR, BATCH_DISP, axis=1) if related else rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    pts = np.array(right_pts, np.float32).reshape(-1, 2)
    pts = pts[rng.permutation(len(pts))]
    kpR = pts + np.float32([0, right_dy])
    kpL = pts + np.float32([BATCH_DISP, 0])
    return imgL, imgR, kpL[:left_n], kpR[:right_n]


def _pack(frames, cap):
    nf = len(frames)
    rows, cols = frames[0][0].shape
    images = np.zeros((nf, 2, rows, cols), np.uint8)
    kp = np.zeros((nf, 2, cap, 2), np.float32)
    n = np.zeros((nf, 2), np.int32)
    for t, (imgL, imgR, kL, kR) in enumerate(frames):
        images[t, 0], images[t, 1] = imgL, imgR
        for side, k in enumerate((kL, kR)):
            assert len(k) <= cap
            kp[t, side, :len(k)] = k
            n[t, side] = len(k)
    return dict(images=images, kp=kp, n=n, cap=cap)


def batch_case(cols, small, rows=BATCH_ROWS):
    """(first, second): two uploads for one Batch.  `first` holds a frame with no right keypoints, a frame whose stereo
    list is empty (unrelated textures, and the right keypoints three rows off the left ones: the stereo matcher accepts
    the best candidate on the epipolar line whatever its cost, so only the absence of candidates empties a list) and
    frames of clearly different list lengths; `second` gives shorter lists (one of them empty where `first` had rows),
    except in the two frames that were empty.  small: cap 5 (one block per frame), a few keypoints on one image row per frame; else
    the whole lattice and a cap that is no multiple of 16."""
    rng = np.random.default_rng(50000 + 10 * cols + small)
    if small:
        cap = 5
        row = lambda y, xs: [(x, y) for x in xs]                 # noqa: E731
        a = [row(7, [20, 6, 7, cols - 8, cols - 7]), row(8, [30, 7]), row(9, [30, 40, 8]), row(6, [9, 7, 50]),
             row(rows - 9, [12, cols - 8, 7, 60]), row(rows - 8, [14, 7, cols - 8])]
        first = [_frame(rng, rows, cols, a[0]), _frame(rng, rows, cols, a[1], right_n=0),
                 _frame(rng, rows, cols, a[2], related=False, right_dy=3), _frame(rng, rows, cols, a[3]),
                 _frame(rng, rows, cols, a[4]), _frame(rng, rows, cols, a[5])]
        second = [_frame(rng, rows, cols, a[0][:3]), _frame(rng, rows, cols, a[1]), _frame(rng, rows, cols, a[2]),
                  _frame(rng, rows, cols, a[3][:2]), _frame(rng, rows, cols, a[4], left_n=0), _frame(rng, rows, cols, a[5][:2])]
    else:
        lat = _lattice(rows, cols)
        cap = len(lat) if len(lat) % 16 else len(lat) + 3
        assert cap > 256                                          # more rows than one sweep of the 16 blocks
        apart = [(x, y) for x, y in lat if y in (0, 8, 20, rows - 8)]     # rows that stay >= 3 apart when one side moves by 3
        first = [_frame(rng, rows, cols, lat), _frame(rng, rows, cols, lat, right_n=0),
                 _frame(rng, rows, cols, apart, related=False, right_dy=3), _frame(rng, rows, cols, lat[::9]),
                 _frame(rng, rows, cols, lat[::2])]
        second = [_frame(rng, rows, cols, lat[::7]), _frame(rng, rows, cols, lat[::11]), _frame(rng, rows, cols, lat[::13]),
                  _frame(rng, rows, cols, lat[::40]), _frame(rng, rows, cols, lat[::5], left_n=0)]
    return _pack(first, cap), _pack(second, cap)


def batch_expected(oracle, case, mode):
    """Per frame (stereo list, refined points): oracle.match_desc on oracle-extracted descriptors, then the restatement."""
    import subpixel_ref as S
    from libviso_amd import hostmath, synth
    from libviso_amd.abi import MatchParams
    st = MatchParams.stereo(hostmath.F_from_P(synth.KITTI_P1, synth.KITTI_P2))
    out = []
    for t in range(len(case["n"])):
        nL, nR = case["n"][t]
        kL, kR = case["kp"][t, 0, :nL], case["kp"][t, 1, :nR]
        imgL, imgR = case["images"][t]
        dL = oracle.extract_descriptors(imgL, kL) if nL else np.zeros((0, 121), np.float32)
        dR = oracle.extract_descriptors(imgR, kR) if nR else np.zeros((0, 121), np.float32)
        m = oracle.match_desc(kL, kR, dL, dR, st) if nL and nR else np.zeros((0, 3), np.int32)
        uv = S.refine(oracle, imgL, imgR, kL, kR, m, mode) if len(m) else np.zeros((0, 2), np.float32)
        out.append((m, uv))
    return out


def batch_fast_counts(case, lists):
    """(fast rows, slow rows) over the frames' lists."""
    rows, cols = case["images"].shape[2:]
    f = np.concatenate([is_fast(row_q(case["kp"][t, 1], m), rows, cols) for t, m in enumerate(lists)] + [np.zeros(0, bool)])
    return int(f.sum()), int((~f).sum())
