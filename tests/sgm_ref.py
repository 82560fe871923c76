"""numpy restatement of the semi-global matching of include/viso_hip.h (viso_stereo_sgm), in exact integers.

sgm() is the vectorised form (the whole cost volume, one path at a time, a row or a column of it per step).  sgm_loop() is a
literal per-pixel, per-path reading of the definition, for small images.  The test pair, the accuracy figures, INVALID and the
PNG helpers are disparity_ref's."""
import numpy as np

from disparity_ref import INVALID, accuracy, kitti_png_values, read_disparity_png, slanted_pair  # noqa: F401

DEFAULTS = dict(num_disp=128, p1=10, p2=120, paths=8, uniqueness=10, lr_max_diff=1)
BIG = 1 << 20
DIRS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1)]   # (dx, dy); the first four with paths = 4


def check_params(num_disp, p1, p2, paths, uniqueness, lr_max_diff):
    return (16 <= num_disp <= 256 and num_disp % 16 == 0 and 1 <= p1 <= p2 <= 192 and paths in (4, 8)
            and 0 <= uniqueness <= 100 and -1 <= lr_max_diff <= num_disp)


def _params(params):
    p = dict(DEFAULTS, **params)
    assert check_params(**p), p
    return tuple(p[k] for k in ("num_disp", "p1", "p2", "paths", "uniqueness", "lr_max_diff"))


def census(img):
    """The 62 bits of the 9 x 7 window (borders replicated) as uint64 [rows][cols]."""
    img = np.asarray(img, np.uint8)
    rows, cols = img.shape
    pad = np.pad(img, ((3, 3), (4, 4)), mode="edge")
    out = np.zeros((rows, cols), np.uint64)
    k = 0
    for j in range(-3, 4):
        for i in range(-4, 5):
            if i == 0 and j == 0:
                continue
            out |= (pad[3 + j:3 + j + rows, 4 + i:4 + i + cols] < img).astype(np.uint64) << np.uint64(k)
            k += 1
    return out


def _popcount(a):
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(a).astype(np.int32)
    b = np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,))
    return np.unpackbits(b, axis=-1).sum(-1).astype(np.int32)


def cost_volume(L, R, D):
    """C [rows][cols][D] int32, BIG where d is not a candidate of the pixel."""
    cL, cR = census(L), census(R)
    rows, cols = cL.shape
    C = np.full((rows, cols, D), BIG, np.int32)
    for d in range(min(D, cols)):
        C[:, d:, d] = _popcount(cL[:, d:] ^ cR[:, :cols - d])
    return C


def sum_volume(L, R, D, P1, P2, paths):
    """S [rows][cols][D] int64 (BIG where d is not a candidate), and the largest S of a candidate."""
    C = cost_volume(L, R, D)
    rows, cols = C.shape[:2]
    cand = C < BIG

    def step(prev, c):   # prev, c: [n][D]; the pixels p - r and p
        mn = prev.min(1, keepdims=True)
        b = np.full_like(prev, BIG)
        b[:, 1:] = prev[:, :-1] + P1
        e = np.full_like(prev, BIG)
        e[:, :-1] = prev[:, 1:] + P1
        r = c + np.minimum(np.minimum(prev, b), np.minimum(e, mn + P2)) - mn
        return np.where(c >= BIG, BIG, r)

    S = np.zeros((rows, cols, D), np.int32)
    for dx, dy in DIRS[:paths]:
        Lr = np.empty_like(C)
        if dy == 0:
            xs = range(cols) if dx > 0 else range(cols - 1, -1, -1)
            for i, x in enumerate(xs):
                Lr[:, x] = C[:, x] if i == 0 else step(Lr[:, x - dx], C[:, x])
        else:
            ys = range(rows) if dy > 0 else range(rows - 1, -1, -1)
            for i, y in enumerate(ys):
                if i == 0:
                    Lr[y] = C[y]
                    continue
                prev = Lr[y - dy]
                if dx == 0:
                    Lr[y] = step(prev, C[y])
                elif dx > 0:
                    Lr[y, 0] = C[y, 0]
                    Lr[y, 1:] = step(prev[:-1], C[y, 1:])
                else:
                    Lr[y, -1] = C[y, -1]
                    Lr[y, :-1] = step(prev[1:], C[y, :-1])
        S += np.where(cand, Lr, 0)
    smax = int(S[cand].max())
    return np.where(cand, S, BIG).astype(np.int64), smax


def select(S, D, u, m):
    """Step 6 of the definition on a finished S (BIG where d is not a candidate)."""
    rows, cols = S.shape[:2]
    cand = S < BIG
    Smin, ds = S.min(2), S.argmin(2)
    valid = np.ones((rows, cols), bool)
    dd = np.arange(D)[None, None, :]
    if u > 0:
        thr = Smin + (Smin * u) // 100
        valid &= ~((cand & (np.abs(dd - ds[..., None]) > 1) & (S <= thr[..., None])).any(2))
    xs = np.arange(cols)[None, :]
    yy, xx = np.mgrid[0:rows, 0:cols]
    if m >= 0:
        keyR = np.full((rows, cols), np.int64(1) << 40, np.int64)
        for d in range(min(D, cols)):
            keyR[:, :cols - d] = np.minimum(keyR[:, :cols - d], (S[:, d:, d] << 8) | d)
        dR = keyR & 0xFF
        valid &= ~(np.abs(dR[yy, xs - ds] - ds) > m)
    dmax = np.minimum(D - 1, xs)
    fit = (ds > 0) & (ds < dmax)
    pp = np.where(fit, S[yy, xx, np.minimum(ds + 1, D - 1)], 0)
    nn = np.where(fit, S[yy, xx, np.maximum(ds - 1, 0)], 0)
    k = pp + nn - 2 * np.where(fit, Smin, 0) + np.abs(pp - nn)
    num = (nn - pp) * 256
    off = np.where(fit & (k > 0), np.abs(num) // np.maximum(k, 1) * np.sign(num), 0)   # C division: truncation toward zero
    out = np.full((rows, cols), INVALID, np.int16)
    d16 = (256 * ds + off + 8) >> 4
    out[valid] = d16[valid].astype(np.int16)
    return out


def sgm(L, R, with_smax=False, **params):
    """int16 [rows][cols] map of the definition (with_smax: also the largest S of any candidate)."""
    D, P1, P2, paths, u, m = _params(params)
    L, R = np.asarray(L, np.uint8), np.asarray(R, np.uint8)
    S, smax = sum_volume(L, R, D, P1, P2, paths)
    out = select(S, D, u, m)
    return (out, smax) if with_smax else out


def sgm_loop(L, R, with_smax=False, **params):
    """Steps 1-6 read literally: pixel by pixel, path by path (small images only)."""
    D, P1, P2, paths, u, m = _params(params)
    L, R = np.asarray(L, np.uint8), np.asarray(R, np.uint8)
    rows, cols = L.shape
    img = {0: L.tolist(), 1: R.tolist()}

    def at(side, x, y):
        return img[side][min(max(y, 0), rows - 1)][min(max(x, 0), cols - 1)]

    def cen(side, x, y):
        c = at(side, x, y)
        return [at(side, x + i, y + j) < c for j in range(-3, 4) for i in range(-4, 5) if (i, j) != (0, 0)]

    cenL = [[cen(0, x, y) for x in range(cols)] for y in range(rows)]
    cenR = [[cen(1, x, y) for x in range(cols)] for y in range(rows)]

    def ncand(x):
        return min(D - 1, x) + 1

    def cost(x, y, d):
        return sum(a != b for a, b in zip(cenL[y][x], cenR[y][x - d]))

    S = [[[0] * ncand(x) for x in range(cols)] for y in range(rows)]
    for dx, dy in DIRS[:paths]:
        Lr = [[None] * cols for _ in range(rows)]
        for y in (range(rows) if dy >= 0 else range(rows - 1, -1, -1)):
            for x in (range(cols) if dx >= 0 else range(cols - 1, -1, -1)):
                C = [cost(x, y, d) for d in range(ncand(x))]
                px, py = x - dx, y - dy
                if not (0 <= px < cols and 0 <= py < rows):
                    Lr[y][x] = C
                    continue
                prev = Lr[py][px]
                M = min(prev)
                cur = []
                for d in range(ncand(x)):
                    terms = [M + P2]
                    if d < len(prev):
                        terms.append(prev[d])
                    if 0 <= d - 1 < len(prev):
                        terms.append(prev[d - 1] + P1)
                    if d + 1 < len(prev):
                        terms.append(prev[d + 1] + P1)
                    cur.append(C[d] + min(terms) - M)
                Lr[y][x] = cur
        for y in range(rows):
            for x in range(cols):
                for d in range(ncand(x)):
                    S[y][x][d] += Lr[y][x][d]

    def dR(xr, y):
        best, bd = None, None
        for d in range(D):
            if xr + d < cols:
                s = S[y][xr + d][d]
                if best is None or s < best:
                    best, bd = s, d
        return bd

    out = np.full((rows, cols), INVALID, np.int16)
    smax = 0
    for y in range(rows):
        for x in range(cols):
            Ss = S[y][x]
            smax = max(smax, max(Ss))
            dmax = len(Ss) - 1
            Sm = min(Ss)
            ds = Ss.index(Sm)
            if u > 0:
                thr = Sm + (Sm * u) // 100
                if any(Ss[d] <= thr for d in range(dmax + 1) if abs(d - ds) > 1):
                    continue
            if m >= 0 and abs(dR(x - ds, y) - ds) > m:
                continue
            off = 0
            if 0 < ds < dmax:
                pp, nn = Ss[ds + 1], Ss[ds - 1]
                k = pp + nn - 2 * Sm + abs(pp - nn)
                if k:
                    num = (nn - pp) * 256
                    off = abs(num) // k * (1 if num >= 0 else -1)
            out[y, x] = (256 * ds + off + 8) >> 4
    return (out, smax) if with_smax else out
