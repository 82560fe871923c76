"""numpy restatement of the dense stereo disparity of include/viso_hip.h (viso_stereo_disparity), in exact integers.

disparity() is the vectorised form (one pass over d for the best disparity and the right image's minima, a second for the
uniqueness test and the sub-pixel neighbours; one int64 cost image per d, never the whole volume).  disparity_loop() is a
literal per-pixel reading of the definition, for small images.  slanted_pair() makes the textured slanted plane the accuracy
tests use."""
import numpy as np

INVALID = -16
DEFAULTS = dict(num_disp=128, block=11, prefilter_cap=31, texture_threshold=10, uniqueness=15, lr_max_diff=1)
BIG = np.int64(1) << 40


def _reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = np.abs(p)
    p = np.where(p >= n, 2 * n - 2 - p, p)
    return p


def sobel_x(img):
    """The extractor's 3x3 Sobel-x, BORDER_REFLECT_101 on both axes: int32 in [-1020, 1020]."""
    I = np.asarray(img, np.int32)
    rows, cols = I.shape
    ym, yp = _reflect101(np.arange(rows) - 1, rows), _reflect101(np.arange(rows) + 1, rows)
    xm, xp = _reflect101(np.arange(cols) - 1, cols), _reflect101(np.arange(cols) + 1, cols)
    h = I[:, xp] - I[:, xm]
    return h[ym] + 2 * h + h[yp]


def prefilter(img, c):
    return np.clip(sobel_x(img), -c, c) + c


def _box(a, r):
    """Sums over the (2r+1)^2 window centred on every pixel whose window lies inside a (other entries 0)."""
    rows, cols = a.shape
    B = 2 * r + 1
    out = np.zeros((rows, cols), np.int64)
    if rows < B or cols < B:
        return out
    s = np.zeros((rows + 1, cols + 1), np.int64)
    s[1:, 1:] = a.cumsum(0).cumsum(1)
    out[r:rows - r, r:cols - r] = s[B:, B:] - s[:-B, B:] - s[B:, :-B] + s[:-B, :-B]
    return out


def _cost(PL, PR, d, r):
    """C(x, y, d) at every inside pixel with x - r - d >= 0 (others meaningless)."""
    diff = np.zeros(PL.shape, np.int64)
    diff[:, d:] = np.abs(PL[:, d:] - PR[:, :PL.shape[1] - d])
    return _box(diff, r)


def check_params(num_disp, block, prefilter_cap, texture_threshold, uniqueness, lr_max_diff):
    return (16 <= num_disp <= 256 and num_disp % 16 == 0 and 5 <= block <= 21 and block % 2 == 1 and 1 <= prefilter_cap <= 63
            and texture_threshold >= 0 and 0 <= uniqueness <= 100 and -1 <= lr_max_diff <= num_disp)


def disparity(L, R, subpixel=True, **params):
    """int16 [rows][cols] map of the definition.  subpixel=False gives 16 d* (the accuracy test's comparison)."""
    p = dict(DEFAULTS, **params)
    assert check_params(**p), p
    D, B, c, T, u, m = (p[k] for k in ("num_disp", "block", "prefilter_cap", "texture_threshold", "uniqueness", "lr_max_diff"))
    r = B // 2
    L, R = np.asarray(L, np.uint8), np.asarray(R, np.uint8)
    rows, cols = L.shape
    out = np.full((rows, cols), INVALID, np.int16)
    if rows < B or cols < B:
        return out
    PL, PR = prefilter(L, c).astype(np.int64), prefilter(R, c).astype(np.int64)
    inside = np.zeros((rows, cols), bool)
    inside[r:rows - r, r:cols - r] = True
    xs = np.arange(cols)[None, :]
    dmax = np.minimum(D - 1, xs - r)
    S = np.full((rows, cols), BIG, np.int64)
    dstar = np.zeros((rows, cols), np.int64)
    keyR = np.full((rows, cols), BIG, np.int64)   # (C << 8) | d of the right pixels
    for d in range(D):
        C = _cost(PL, PR, d, r)
        cand = inside & (d <= dmax)
        if not cand.any():
            break
        better = cand & (C < S)
        S = np.where(better, C, S)
        dstar = np.where(better, d, dstar)
        # right pixel xr = x - d gets the left pixel x's key
        key = np.where(cand, (C << 8) | d, BIG)
        keyR[:, :cols - d] = np.minimum(keyR[:, :cols - d], key[:, d:])
    valid = inside.copy()
    tex = _box(np.abs(PL - c), r)
    valid &= tex >= T
    n_ = np.full((rows, cols), BIG, np.int64)
    p_ = np.full((rows, cols), BIG, np.int64)
    thr = S + (S * u) // 100
    for d in range(D):
        cand = inside & (d <= dmax)
        if not cand.any():
            break
        C = _cost(PL, PR, d, r)
        n_ = np.where(cand & (d == dstar - 1), C, n_)
        p_ = np.where(cand & (d == dstar + 1), C, p_)
        if u > 0:
            valid &= ~(cand & (np.abs(d - dstar) > 1) & (C <= thr))
    if m >= 0:
        dR = keyR & 0xFF
        yy = np.arange(rows)[:, None].repeat(cols, 1)
        xr = np.clip(xs - dstar, 0, cols - 1)
        valid &= ~(inside & (np.abs(dR[yy, xr] - dstar) > m))
    off = np.zeros((rows, cols), np.int64)
    if subpixel:
        fit = valid & (dstar > 0) & (dstar < dmax)
        pp, nn = np.where(fit, p_, 0), np.where(fit, n_, 0)
        k = pp + nn - 2 * np.where(fit, S, 0) + np.abs(pp - nn)
        num = (nn - pp) * 256
        q = np.where(k > 0, np.abs(num) // np.maximum(k, 1), 0) * np.sign(num)   # C division: truncation toward zero
        off = np.where(fit, q, 0)
    disp16 = (256 * dstar + off + 8) >> 4
    out[valid] = disp16[valid].astype(np.int16)
    return out


def disparity_loop(L, R, **params):
    """Steps 1-9 read literally, pixel by pixel (small images only)."""
    p = dict(DEFAULTS, **params)
    assert check_params(**p), p
    D, B, c, T, u, m = (p[k] for k in ("num_disp", "block", "prefilter_cap", "texture_threshold", "uniqueness", "lr_max_diff"))
    r = B // 2
    rows, cols = L.shape
    out = np.full((rows, cols), INVALID, np.int16)
    PL, PR = prefilter(L, c).tolist(), prefilter(R, c).tolist()

    def cost(x, y, d):
        return sum(abs(PL[y + j][x + i] - PR[y + j][x + i - d]) for j in range(-r, r + 1) for i in range(-r, r + 1))

    def inside(x, y):
        return r <= y < rows - r and r <= x < cols - r

    def dR(xr, y):
        best, bd = None, None
        for d in range(D):
            if xr + d < cols - r:
                cc = cost(xr + d, y, d)
                if best is None or cc < best:
                    best, bd = cc, d
        return bd

    for y in range(rows):
        for x in range(cols):
            if not inside(x, y):
                continue
            dmax = min(D - 1, x - r)
            Cs = [cost(x, y, d) for d in range(dmax + 1)]
            S = min(Cs)
            ds = Cs.index(S)
            if sum(abs(PL[y + j][x + i] - c) for j in range(-r, r + 1) for i in range(-r, r + 1)) < T:
                continue
            if u > 0:
                thr = S + (S * u) // 100
                if any(Cs[d] <= thr for d in range(dmax + 1) if abs(d - ds) > 1):
                    continue
            if m >= 0 and abs(dR(x - ds, y) - ds) > m:
                continue
            off = 0
            if 0 < ds < dmax:
                pp, nn = Cs[ds + 1], Cs[ds - 1]
                k = pp + nn - 2 * S + abs(pp - nn)
                if k:
                    num = (nn - pp) * 256
                    off = abs(num) // k * (1 if num >= 0 else -1)
            out[y, x] = (256 * ds + off + 8) >> 4
    return out


def _texture_row(rng, n):
    """A band-limited random texture along one row: integer knots every pixel, blurred, for linear interpolation."""
    t = rng.normal(size=n + 8)
    k = np.exp(-0.5 * (np.arange(-3, 4) / 1.0) ** 2)
    return np.convolve(t, k / k.sum(), mode="same")


def slanted_pair(rows=376, cols=1241, dmin=8.0, dmax=78.0, noise=1.0, seed=0):
    """A textured slanted plane: left image L(x, y) = T(x, y), right image R(xr, y) = T(xr + dL, y) where the true left
    disparity dL(x, y) = a + b x + c y runs from dmin to dmax.  Returns (L, R, true disparity of the left pixels)."""
    rng = np.random.default_rng(seed)
    b = (dmax - dmin) * 0.7 / (cols - 1)
    cy = (dmax - dmin) * 0.3 / (rows - 1)
    a = dmin
    ys, xs = np.mgrid[0:rows, 0:cols].astype(np.float64)
    dtrue = a + b * xs + cy * ys
    W = cols + 2 * int(dmax) + 16
    tex = np.stack([_texture_row(rng, W) for _ in range(rows)])
    tex = (tex - tex.mean()) / tex.std()
    tex = 0.5 * tex + 0.5 * np.roll(tex, 1, axis=0)   # some vertical correlation

    def sample(u):   # T at real positions u (per row), linear interpolation
        u = u + 8
        i0 = np.floor(u).astype(np.int64)
        f = u - i0
        row = np.arange(rows)[:, None]
        return tex[row, i0] * (1 - f) + tex[row, i0 + 1] * f

    left = sample(xs)
    # right pixel xr sees the scene point whose left column x solves x - dL(x, y) = xr
    xl = (xs + a + cy * ys) / (1.0 - b)
    right = sample(xl)
    L = np.clip(np.rint(128 + 40 * left + rng.normal(scale=noise, size=left.shape)), 0, 255).astype(np.uint8)
    R = np.clip(np.rint(128 + 40 * right + rng.normal(scale=noise, size=right.shape)), 0, 255).astype(np.uint8)
    return L, R, dtrue


def accuracy(d16, dtrue):
    """(share of valid pixels, median |error| px, share of valid pixels with |error| > 1 px)."""
    v = d16 != INVALID
    err = np.abs(d16[v] / 16.0 - dtrue[v])
    return v.mean(), float(np.median(err)), float((err > 1.0).mean())


def read_disparity_png(path):
    """A KITTI stereo PNG (16-bit grayscale) decoded with Python's zlib, every chunk's CRC-32 checked (zlib checks the Adler-32).
    Returns the uint16 values [rows][cols]."""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, ihdr, chunks = 8, b"", None, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert zlib.crc32(kind + body) == crc, kind
        chunks.append(kind)
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    assert chunks[0] == b"IHDR" and chunks[-1] == b"IEND" and pos == len(data)
    cols, rows, depth, color, comp, filt, inter = ihdr
    assert (depth, color, comp, filt, inter) == (16, 0, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(rows, 2 * cols + 1)
    assert (raw[:, 0] == 0).all()   # filter 0 on every row
    return raw[:, 1:].copy().view(">u2").astype(np.uint16)


def kitti_png_values(d16):
    """What viso_write_disparity_png stores: 16 * disp16 for valid pixels, 0 for invalid ones."""
    d16 = np.asarray(d16, np.int32)
    return np.where(d16 < 0, 0, 16 * d16).astype(np.uint16)
