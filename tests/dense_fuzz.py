"""Random geometries, parameters and image classes for the dense image stage, each kernel's direct call against its numpy
restatement: rectify_images (tests/rectify_ref.py), stereo_disparity (tests/disparity_ref.py), stereo_sgm (tests/sgm_ref.py),
filter_speckles and disparity_to_points (tests/speckle_ref.py).  The shapes are drawn from mixtures that sit on the places where
the kernels split their work (thread runs and the 64 KiB LDS line of the block matcher, the lanes' K disparities and the diagonal
wrap of SGM, the 64 x 16 speckle tile, the 1024-pixel tile and the 32-frame chunk of the remap), the parameters over the whole
range the *_params_ok checks accept with the end values over-weighted.

Test infrastructure: lives under tests/.  The generators need numpy alone (no device, no library); tests/test_dense_fuzz_cpu.py
checks on the restatements that they reach every seam, tests/test_gpu_dense_fuzz.py runs SEEDS x COUNTS on the device.  As a
script (not collected by pytest) it runs N cases of every kernel and prints what differs:  python3 tests/dense_fuzz.py SEED N"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

INVALID = -16
KERNELS = ("bm", "sgm", "speckle", "rectify", "points")

# What tests/test_gpu_dense_fuzz.py runs and tests/test_dense_fuzz_cpu.py checks the coverage of: cases(seed, COUNTS[kernel]) for
# every seed.  The counts are sized by the restatement's time (the figures are in the docstring of test_gpu_dense_fuzz.py).
SEEDS = (0, 1, 2)
COUNTS = dict(bm=150, sgm=160, speckle=300, rectify=100, points=150)

# ---- the ranges the generators draw from (the parameter checks of test_gpu_dense_fuzz.py step one past each of them) ---------
BLOCKS = tuple(range(5, 22, 2))                     # the nine odd blocks
NUM_DISPS = tuple(range(16, 257, 16))               # the sixteen disparity counts
CAP_RANGE = (1, 63)                                 # prefilter_cap
UNIQ_RANGE = (0, 100)
P_RANGE = (1, 192)                                  # 1 <= p1 <= p2 <= 192
PATHS = (4, 8)
MAX_DIFFS = (0, 1, 16, 4096)
MAX_DIFF_RANGE = (0, 4096)
BORDER_RANGE = (0, 255)
TEX_HUGE = (1 << 31) - 1

DISP_THREADS, DISP_MAX_COLS = 256, 2048             # disparity.hip
RECT_TILE, RECT_FPB = 1024, 32                      # rectify.hip
SPK_TW, SPK_TH = 64, 16                             # speckle.hip
WIDTH_SEAMS = tuple(256 * k + e for k in range(1, 9) for e in (-1, 0, 1) if 256 * k + e <= DISP_MAX_COLS)
FRAME_COUNTS = (1, 2, 31, 32, 33, 64, 65)

_TAGS = dict(bm=11, sgm=12, speckle=13, rectify=14, points=15)


def _rng(kind, seed, i):
    """Every case has its own generator: case i of a seed is the same whatever n is and whichever cases came before it."""
    return np.random.default_rng([_TAGS[kind], int(seed), int(i)])


def _pick(rng, values, p=None):
    return values[int(rng.choice(len(values), p=p))]


def _ends_or_random(rng, ends, lo, hi, p_ends=0.5):
    """One of the end values with probability p_ends, else uniform in lo .. hi."""
    return int(_pick(rng, ends)) if rng.random() < p_ends else int(rng.integers(lo, hi + 1))


# ---- geometry of the block matcher (disparity.hip) -----------------------------------------------------------------------------
def bm_run(cols):
    """Columns per thread of stereo_disparity_kernel."""
    return (cols + DISP_THREADS - 1) // DISP_THREADS


def bm_k(block):
    """Packed dwords per column of stereo_disparity_kernel."""
    return (block + 3) // 4


def bm_lds_bytes(block, cols):
    return 4 * (2 * bm_k(block) + 2) * cols


def bm_above_lds_line(block, cols):
    """The launch asks for more dynamic LDS than the 64 KiB a kernel gets without the attribute."""
    return bm_lds_bytes(block, cols) > 65536


def sgm_k(num_disp):
    """Disparities per lane of sgm_path_kernel."""
    return (num_disp + 63) // 64


# ---- images --------------------------------------------------------------------------------------------------------------------
IMAGE_CLASSES = ("textured", "constant", "stripes", "checker", "midgray", "black-white", "identical")
_IMAGE_P = (0.46, 0.04, 0.09, 0.09, 0.11, 0.11, 0.10)


def image_pair(rng, rows, cols):
    """(class, L, R) of one size: the classes of the issue (every rule of the selection has work in one of them)."""
    from test_gpu_disparity import _pair
    cls = _pick(rng, IMAGE_CLASSES, _IMAGE_P)
    shift = 0 if rng.random() < 0.15 else int(rng.integers(1, 41))
    yy, xx = np.mgrid[0:rows, 0:cols]
    if cls == "textured":
        L, R = _pair(rng, rows, cols, shift)
    elif cls == "constant":
        L = np.full((rows, cols), int(rng.integers(0, 256)), np.uint8)
        R = L.copy() if rng.random() < 0.5 else np.full((rows, cols), int(rng.integers(0, 256)), np.uint8)
    elif cls in ("stripes", "checker"):
        period = int(rng.integers(2, 9))
        a, b = (int(v) for v in rng.integers(0, 256, 2))

        def pat(x):
            on = (x % period) * 2 < period
            if cls == "checker":
                on = on ^ ((yy % period) * 2 < period)
            return np.where(on, a, b).astype(np.uint8)
        L, R = pat(xx), pat(xx + shift)          # a right pixel x sees what the left pixel x + shift sees
    elif cls == "midgray":
        L = (128 + rng.integers(-1, 2, (rows, cols))).astype(np.uint8)
        R = (128 + rng.integers(-1, 2, (rows, cols))).astype(np.uint8) if rng.random() < 0.5 else np.roll(L, -shift, 1)
    elif cls == "black-white":
        L = (rng.integers(0, 2, (rows, cols)) * 255).astype(np.uint8)
        R = (rng.integers(0, 2, (rows, cols)) * 255).astype(np.uint8) if rng.random() < 0.5 else np.roll(L, -shift, 1)
    else:
        L, _ = _pair(rng, rows, cols, shift)
        R = L.copy()
    return cls, np.ascontiguousarray(L, dtype=np.uint8), np.ascontiguousarray(R, dtype=np.uint8)


def _uniq(rng):
    """0, 1, 99 and 100 over-weighted; the rest of 0 .. 100 with the small ratios more often (a large one leaves few pixels valid)."""
    if rng.random() < 0.3:
        return int(_pick(rng, (0, 1, 99, 100), (0.3, 0.3, 0.2, 0.2)))
    return int((UNIQ_RANGE[1] + 1) * rng.random() ** 3)


def _lr(rng, D):
    return _ends_or_random(rng, (-1, 0, 1, D), -1, D, p_ends=0.6)


# ---- block matching ------------------------------------------------------------------------------------------------------------
def bm_cases(seed, n):
    """n cases of stereo_disparity: dict(kind, seed, index, geometry, image, L, R, params)."""
    for i in range(n):
        rng = _rng("bm", seed, i)
        B = int(_pick(rng, BLOCKS))
        D = int(_pick(rng, NUM_DISPS))
        g = rng.random()
        if g < 0.30:       # a width at a multiple of the 256 threads, +- 1: the last threads' runs are empty or partial
            geometry = "width seam"
            cols = WIDTH_SEAMS[(i + 7 * seed) % len(WIDTH_SEAMS)]   # in turn: every width comes up, whatever the other draws
            rows = B + int(rng.integers(0, 3))
        elif g < 0.38:     # above the 64 KiB dynamic-LDS line: cols > 16384 / (2K + 2), K >= 4
            geometry = "LDS line"
            if rng.random() < 0.3:
                B, cols = 21, 1241
            else:
                B = int(_pick(rng, (13, 15, 17, 19, 21)))
                first = 16384 // (2 * bm_k(B) + 2) + 1
                cols = first + int(rng.integers(0, 3)) if rng.random() < 0.5 else int(rng.integers(first, DISP_MAX_COLS + 1))
            rows = B + int(rng.integers(0, 2))
        elif g < 0.44:     # around the window
            geometry = "window"
            cols = max(1, B + int(rng.integers(-2, 3)))
            rows = max(1, B + int(rng.integers(-1, 4)))
        else:
            geometry = "general"
            cols = int(rng.integers(1, 401))
            h = rng.random()
            rows = 1 if h < 0.02 else B - 1 if h < 0.05 else B if h < 0.22 else B + 1 if h < 0.40 else int(rng.integers(
                1, 49)) if h < 0.55 else int(rng.integers(B, B + 28))
        if geometry in ("width seam", "LDS line") and cols > 1100 and rng.random() < 0.75:
            D = int(_pick(rng, NUM_DISPS[:4]))   # the restatement walks every d over the whole row: mostly few of them when it is wide
        cls, L, R = image_pair(rng, rows, cols)
        cap = _ends_or_random(rng, (1, 2, 62, 63), *CAP_RANGE, p_ends=0.4)
        t = rng.random()   # small: below a quarter of the largest texture sum c B^2; huge: above every sum
        tex = 0 if t < 0.35 else 1 if t < 0.5 else int(rng.integers(2, max(3, cap * B * B // 4))) if t < 0.96 else int(
            _pick(rng, (10 ** 6, TEX_HUGE)))
        params = dict(num_disp=D, block=B, prefilter_cap=cap, texture_threshold=tex, uniqueness=_uniq(rng), lr_max_diff=_lr(rng, D))
        yield dict(kind="bm", seed=seed, index=i, geometry=geometry, image=cls, L=L, R=R, params=params)


# ---- semi-global matching ------------------------------------------------------------------------------------------------------
def sgm_cases(seed, n):
    """n cases of stereo_sgm: dict(kind, seed, index, geometry, image, L, R, params)."""
    for i in range(n):
        rng = _rng("sgm", seed, i)
        D = int(_pick(rng, NUM_DISPS))
        g = rng.random()
        if g < 0.25:       # the census grid's and the select kernel's 256 stride
            geometry = "width seam"
            cols, rows = WIDTH_SEAMS[(i + 7 * seed) % len(WIDTH_SEAMS)], int(rng.integers(1, 5))
            if cols > 1100 and rng.random() < 0.6:
                D = int(_pick(rng, NUM_DISPS[:4]))
        elif g < 0.34:     # around the 9 x 7 census window
            geometry = "window"
            cols, rows = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        elif g < 0.46:     # tall and narrow: a diagonal line wraps several times
            geometry = "tall narrow"
            cols, rows = int(rng.integers(1, 6)), int(rng.integers(6, 41))
        else:
            geometry = "general"
            cols, rows = int(rng.integers(1, 401)), int(rng.integers(1, 17))
        cls, L, R = image_pair(rng, rows, cols)
        h = rng.random()
        if h < 0.12:
            p1, p2 = 1, 1
        elif h < 0.30:     # p1 = p2, the ends among them
            p1 = p2 = _ends_or_random(rng, (191, 192), *P_RANGE, p_ends=0.5)
        elif h < 0.50:
            p2 = int(_pick(rng, (191, 192)))
            p1 = int(rng.integers(1, p2 + 1))
        else:
            p1 = int(rng.integers(P_RANGE[0], P_RANGE[1] + 1))
            p2 = int(rng.integers(p1, P_RANGE[1] + 1))
        params = dict(num_disp=D, p1=p1, p2=p2, paths=int(_pick(rng, PATHS)), uniqueness=_uniq(rng), lr_max_diff=_lr(rng, D))
        yield dict(kind="sgm", seed=seed, index=i, geometry=geometry, image=cls, L=L, R=R, params=params)


# ---- speckle filter ------------------------------------------------------------------------------------------------------------
def speckle_cases(seed, n):
    """n cases of filter_speckles: dict(kind, seed, index, geometry, image, map, params, size_of), size_of the component size that
    max_size was taken from (None: 0, 1 or rows * cols)."""
    import speckle_ref as K
    from test_speckle_cpu import random_map
    for i in range(n):
        rng = _rng("speckle", seed, i)
        g = rng.random()
        if g < 0.70:       # around multiples of the 16 x 64 tile
            geometry = "tile seam"
            rows = SPK_TH * int(rng.integers(1, 4)) + int(rng.integers(-1, 2))
            cols = SPK_TW * int(rng.integers(1, 5)) + int(rng.integers(-1, 2))
        elif g < 0.80:
            geometry, rows, cols = "one row", 1, int(rng.integers(1, 301))
        elif g < 0.90:
            geometry, rows, cols = "one column", int(rng.integers(1, 301)), 1
        else:
            geometry, rows, cols = "general", int(rng.integers(1, 61)), int(rng.integers(1, 301))
        max_diff = int(_pick(rng, MAX_DIFFS))
        s = rng.random()
        if s < 0.12 and rows > 2 and cols > 2:
            # one thin component over the whole map, with single pixels in its gaps that must not join it
            cls = _pick(rng, ("serpentine", "vertical serpentine", "comb"))
            m, _ = K.comb(rows, cols) if cls == "comb" else K.serpentine(rows, cols, vertical=cls.startswith("vertical"))
            m[(m == INVALID) & (rng.random(m.shape) < 0.2)] = 320 + max_diff + 1 + int(rng.integers(0, 2000))
        else:
            spread = int(_pick(rng, (2, 6, 40, 2000, 8000)))
            invalid = float(rng.random() * 0.7)
            cls = "random spread %d invalid %.3f" % (spread, invalid)
            m = random_map(rng, rows, cols, spread=spread, invalid=invalid)
            e = rng.random()
            if e < 0.10:       # the ends of the int16 range (a value that lands on INVALID is an invalid pixel like any other)
                m = np.where(m == INVALID, INVALID, m.astype(np.int32) + (32767 - (spread - 1))).astype(np.int16)
                cls += " at +32767"
            elif e < 0.20:
                m = np.where(m == INVALID, INVALID, m.astype(np.int32) - 32768).astype(np.int16)
                cls += " at -32768"
        sz = K.component_sizes(m, max_diff)
        sizes = np.unique(sz[sz > 0])
        size_of = None
        c = rng.random()
        if c < 0.70 and sizes.size:
            size_of = int(_pick(rng, sizes))
            max_size = size_of - 1 if c < 0.33 else size_of
        else:
            max_size = int(_pick(rng, (0, 1, rows * cols)))
        yield dict(kind="speckle", seed=seed, index=i, geometry=geometry, image=cls, map=np.ascontiguousarray(m, dtype=np.int16),
                   params=dict(max_size=max_size, max_diff=max_diff), size_of=size_of)


# ---- rectification -------------------------------------------------------------------------------------------------------------
def hostile_map(rng, raw_shape, out_shape):
    """Positions reaching 0-2.5 px past every edge, negative ones, entries exactly at raw_cols-1 / raw_rows-1 (partial taps),
    all 32 fractions, NaN, +-inf and +-40000."""
    rr, rc = raw_shape
    mx = rng.uniform(-2.5, rc + 1.5, out_shape).astype(np.float32)
    my = rng.uniform(-2.5, rr + 1.5, out_shape).astype(np.float32)
    fl = mx.reshape(-1); gl = my.reshape(-1)
    n = fl.size
    k = np.arange(n)
    frac = (k % 32).astype(np.float32) / np.float32(32)
    sel = k % 5 == 0                                    # exact 1/32 fractions on integer bases
    fl[sel] = np.floor(fl[sel]) + frac[sel]
    gl[sel] = np.floor(gl[sel]) + frac[(k[sel] * 7) % n]
    special = [np.nan, np.inf, -np.inf, 40000.0, -40000.0, rc - 1, -1.0, -0.5, rc - 1 + 0.5, 0.0]
    for j, v in enumerate(special):
        if 3 * j + 2 < n:
            fl[3 * j + 1] = v
            gl[3 * j + 2] = {rc - 1: rr - 1, rc - 1 + 0.5: rr - 1 + 0.5}.get(v, v)
    return mx, my


def rectify_cases(seed, n):
    """n cases of rectify_images: dict(kind, seed, index, geometry, raw [nf][rr][rc], mapx, mapy, out_shape, border)."""
    for i in range(n):
        rng = _rng("rectify", seed, i)
        if rng.random() < 0.55:   # output pixels around multiples of the 1024-pixel tile
            geometry = "tile seam"
            per = RECT_TILE * int(rng.integers(1, 4)) + int(rng.integers(-3, 4))
        else:
            geometry = "general"
            per = int(rng.integers(1, 601))
        divisors = [d for d in range(1, 65) if per % d == 0]
        out_rows = int(_pick(rng, divisors))
        out_shape = (out_rows, per // out_rows)
        raw_shape = (int(rng.integers(1, 31)), int(rng.integers(1, 45)))
        nf = int(_pick(rng, FRAME_COUNTS))
        raw = rng.integers(0, 256, (nf,) + raw_shape, dtype=np.uint8)
        mapx, mapy = hostile_map(rng, raw_shape, out_shape)
        border = _ends_or_random(rng, BORDER_RANGE, *BORDER_RANGE, p_ends=0.3)
        yield dict(kind="rectify", seed=seed, index=i, geometry=geometry, image="hostile map", raw=raw, mapx=mapx, mapy=mapy,
                   out_shape=out_shape, border=border)


# ---- reprojection --------------------------------------------------------------------------------------------------------------
def points_cases(seed, n):
    """n cases of disparity_to_points: dict(kind, seed, index, geometry, image, map, calib (base, f, cu, cv), pose, min_disp16)."""
    from libviso_amd import hostmath
    from test_speckle_cpu import random_map
    for i in range(n):
        rng = _rng("points", seed, i)
        g = rng.random()
        if g < 0.4:        # pixel counts around multiples of the 256 threads
            geometry = "block seam"
            px = 256 * int(rng.integers(1, 9)) + int(rng.integers(-1, 2))
            rows = int(_pick(rng, [d for d in range(1, 65) if px % d == 0]))
            cols = px // rows
        elif g < 0.5:
            geometry, rows, cols = "one row", 1, int(rng.integers(1, 600))
        elif g < 0.6:
            geometry, rows, cols = "one column", int(rng.integers(1, 600)), 1
        else:
            geometry, rows, cols = "general", int(rng.integers(1, 80)), int(rng.integers(1, 400))
        spread = int(_pick(rng, (40, 400, 2100, 32000)))
        invalid = float(rng.random() * 0.6)
        m = random_map(rng, rows, cols, spread=spread, invalid=invalid)
        low = rng.random((rows, cols)) < 0.1            # 0 (never divides), small and negative values
        m[low] = rng.integers(-40, 20, int(low.sum())).astype(np.int16)
        min_disp16 = _ends_or_random(rng, (1, 16, 160), 1, 400, p_ends=0.6)
        calib = dict(base=float(rng.uniform(0.1, 1.0)), f=float(rng.uniform(300.0, 1000.0)), cu=float(rng.uniform(0.0, cols + 1.0)),
                     cv=float(rng.uniform(0.0, rows + 1.0)))
        q = rng.random()
        pose = None if q < 0.35 else np.eye(4) if q < 0.45 else np.linalg.inv(hostmath.tr2mat(
            np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 1.0, 3)])))
        if pose is not None and rng.random() < 0.3:
            pose = np.ascontiguousarray(pose[:3])
        yield dict(kind="points", seed=seed, index=i, geometry=geometry, image="random spread %d invalid %.3f" % (spread, invalid),
                   map=np.ascontiguousarray(m, dtype=np.int16), calib=calib, pose=pose, min_disp16=min_disp16)


CASES = dict(bm=bm_cases, sgm=sgm_cases, speckle=speckle_cases, rectify=rectify_cases, points=points_cases)


# ---- a case: its words, its bytes, its two sides ---------------------------------------------------------------------------------
def describe(case):
    """Everything needed to run the case again: next(itertools.islice(CASES[kind](seed, index + 1), index, None))."""
    k = case["kind"]
    head = "%s seed %d index %d (%s, %s)" % (k, case["seed"], case["index"], case["geometry"], case["image"])
    if k in ("bm", "sgm"):
        return "%s: %d x %d, %s" % (head, case["L"].shape[0], case["L"].shape[1], case["params"])
    if k == "speckle":
        return "%s: %d x %d, %s, from a component of %s pixels" % (head, case["map"].shape[0], case["map"].shape[1], case["params"],
                                                                   case["size_of"])
    if k == "rectify":
        return "%s: %d frames of raw %d x %d -> out %d x %d (%d pixels), border %d" % (
            (head, case["raw"].shape[0]) + case["raw"].shape[1:] + tuple(case["out_shape"])
            + (case["out_shape"][0] * case["out_shape"][1], case["border"]))
    pose = "no pose" if case["pose"] is None else "pose %s" % np.asarray(case["pose"]).reshape(-1).tolist()
    return "%s: %d x %d, min_disp16 %d, %s, %s" % (head, case["map"].shape[0], case["map"].shape[1], case["min_disp16"], case["calib"], pose)


def case_digest(case):
    """A hash over every byte of the case: the arrays' types, shapes and contents, and the words of everything else."""
    h = hashlib.sha256()
    for key in sorted(case):
        v = case[key]
        h.update(key.encode())
        if isinstance(v, np.ndarray):
            h.update(str((v.dtype, v.shape)).encode())
            h.update(np.ascontiguousarray(v).tobytes())
        elif isinstance(v, dict):
            h.update(repr(sorted(v.items())).encode())
        else:
            h.update(repr(v).encode())
    return h.hexdigest()


def _calib(case):
    from libviso_amd.abi import Param
    return Param.default(**case["calib"])


def expected(case):
    """The restatement's output of the case."""
    k = case["kind"]
    if k == "bm":
        import disparity_ref as DR
        return DR.disparity(case["L"], case["R"], **case["params"])
    if k == "sgm":
        import sgm_ref as SR
        return SR.sgm(case["L"], case["R"], **case["params"])
    import speckle_ref as K
    if k == "speckle":
        return K.speckles(case["map"], case["params"]["max_size"], case["params"]["max_diff"])
    if k == "rectify":
        import rectify_ref as RR
        return np.stack([RR.remap(r, case["mapx"], case["mapy"], case["border"]) for r in case["raw"]])
    return K.points(case["map"], _calib(case), case["pose"], case["min_disp16"])


def device(case):
    """The direct call's output of the case."""
    import libviso_amd
    k = case["kind"]
    if k == "bm":
        return libviso_amd.stereo_disparity(case["L"], case["R"], **case["params"])
    if k == "sgm":
        return libviso_amd.stereo_sgm(case["L"], case["R"], **case["params"])
    if k == "speckle":
        return libviso_amd.filter_speckles(case["map"], **case["params"])
    if k == "rectify":
        return libviso_amd.rectify_images(case["raw"], case["mapx"], case["mapy"], case["out_shape"], border=case["border"])
    return libviso_amd.disparity_to_points(case["map"], _calib(case), pose=case["pose"], min_disp16=case["min_disp16"])


def same(case, got, want):
    """Exact: np.array_equal on the integer outputs; the points bit for bit with one NaN mask (tests/test_gpu_points.py)."""
    if case["kind"] == "points":
        import speckle_ref as K
        use = (case["map"] != INVALID) & (case["map"] >= case["min_disp16"])
        return got.dtype == np.float32 and K.points_equal(got, want) and np.array_equal(np.isfinite(got[..., 2]), use)
    return got.dtype == want.dtype and np.array_equal(got, want)


def mismatches(kind, seed, n):
    """describe() of every case of CASES[kind](seed, n) whose device output is not the restatement's."""
    bad = []
    for case in CASES[kind](seed, n):
        got, want = device(case), expected(case)
        if not same(case, got, want):
            bad.append(describe(case) + ": %d of %d values differ" % (
                int((got != want).sum()) if got.shape == want.shape and case["kind"] != "points" else -1, want.size))
    return bad


if __name__ == "__main__":
    import time

    import libviso_amd
    libviso_amd.load()
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    t0 = time.time()
    n_bad = 0
    for kind in KERNELS:   # n cases of every kernel
        t1 = time.time()
        bad = mismatches(kind, seed, n)
        for b in bad[:40]:
            print("MISMATCH", b, flush=True)
        n_bad += len(bad)
        print("%s: %d cases, %d mismatches, %.1f s" % (kind, n, len(bad), time.time() - t1), flush=True)
    print("done, seed %d: mismatches: %d, %.1f s" % (seed, n_bad, time.time() - t0))
    sys.exit(1 if n_bad else 0)
