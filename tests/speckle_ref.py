"""numpy restatements of the speckle filter and the reprojection of include/viso_hip.h ("speckle filter and 3-D reprojection of the
maps"): the oracle of libviso_amd/csrc/speckle.hip.  `speckles` finds the components by hooking and pointer jumping over the list
of links; `speckles_loop` is a literal flood fill, pixel by pixel, in the order OpenCV's filterSpeckles walks; `points` writes
the reprojection's association out.  numpy only."""
import numpy as np

INVALID = -16   # VISO_DISP_INVALID


def links(m, max_diff):
    """(hor [rows][cols-1], ver [rows-1][cols]) bool: pixel (y, x) linked to (y, x+1) / to (y+1, x)."""
    m = np.asarray(m)
    v, mi = m != INVALID, m.astype(np.int32)
    hor = v[:, 1:] & v[:, :-1] & (np.abs(mi[:, 1:] - mi[:, :-1]) <= max_diff)
    ver = v[1:, :] & v[:-1, :] & (np.abs(mi[1:, :] - mi[:-1, :]) <= max_diff)
    return hor, ver


def labels(m, max_diff):
    """int64 [rows][cols]: the smallest linear index of every pixel's component (an invalid pixel: its own index)."""
    m = np.asarray(m)
    rows, cols = m.shape
    idx = np.arange(rows * cols, dtype=np.int64).reshape(rows, cols)
    hor, ver = links(m, max_diff)
    a = np.concatenate([idx[:, 1:][hor], idx[1:, :][ver]])
    b = np.concatenate([idx[:, :-1][hor], idx[:-1, :][ver]])
    L = idx.ravel().copy()
    while a.size:
        la, lb = L[a], L[b]                      # roots: L is flat here
        differ = la != lb
        a, b, la, lb = a[differ], b[differ], la[differ], lb[differ]
        if not a.size:
            break
        np.minimum.at(L, np.maximum(la, lb), np.minimum(la, lb))   # hook the larger root under the smaller
        while True:                              # pointer jumping until every pixel points at its root
            L2 = L[L]
            if np.array_equal(L2, L):
                break
            L = L2
    return L.reshape(rows, cols)


def component_sizes(m, max_diff):
    """int64 [rows][cols]: the pixel count of every valid pixel's component, 0 at invalid pixels."""
    m = np.asarray(m)
    L = labels(m, max_diff)
    valid = m != INVALID
    cnt = np.bincount(L[valid], minlength=m.size)
    return np.where(valid, cnt[L], 0)


def speckles(m, max_size, max_diff):
    """The filtered copy of the int16 map m."""
    m = np.asarray(m)
    assert m.dtype == np.int16 and m.ndim == 2 and max_size >= 0 and 0 <= max_diff <= 4096
    out = m.copy()
    sz = component_sizes(m, max_diff)
    out[(m != INVALID) & (sz <= max_size)] = INVALID
    return out


def speckles_loop(m, max_size, max_diff):
    """filterSpeckles(img, newVal = INVALID, maxSpeckleSize = max_size, maxDiff = max_diff) as OpenCV walks it: rows top to bottom,
    pixels left to right; an unlabelled valid pixel starts a flood fill from a stack, each popped pixel looking down, up, right, left
    and comparing the neighbour with ITS OWN value; a region of at most max_size pixels is marked small and set to newVal, and later
    pixels that meet a small region's label are set to newVal too."""
    m = np.asarray(m)
    rows, cols = m.shape
    out = m.copy()
    lab = np.zeros((rows, cols), np.int64)
    small = [False]
    cur = 0
    for i in range(rows):
        for j in range(cols):
            if out[i, j] == INVALID:
                continue
            if lab[i, j]:
                if small[lab[i, j]]:
                    out[i, j] = INVALID
                continue
            cur += 1
            lab[i, j] = cur
            stack, count = [(i, j)], 0
            while stack:
                y, x = stack.pop()
                count += 1
                dp = int(m[y, x])
                for yy, xx in ((y + 1, x), (y - 1, x), (y, x + 1), (y, x - 1)):
                    if 0 <= yy < rows and 0 <= xx < cols and not lab[yy, xx] and m[yy, xx] != INVALID and abs(dp - int(m[yy, xx])) <= max_diff:
                        lab[yy, xx] = cur
                        stack.append((yy, xx))
            small.append(count <= max_size)
            if small[cur]:
                out[i, j] = INVALID
    return out


def points(m, param, pose=None, min_disp16=1):
    """float32 [rows][cols][3] of include/viso_hip.h: param has f, cu, cv, base; pose None or a 4 x 4 (3 x 4) float64 matrix."""
    m = np.asarray(m)
    assert m.dtype == np.int16 and m.ndim == 2 and min_disp16 >= 1
    rows, cols = m.shape
    use = (m != INVALID) & (m >= min_disp16)
    f, cu, cv, base = (np.float64(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = m.astype(np.float64) / 16.0
        X = (base * (x - cu)) / d
        Y = (base * (y - cv)) / d
        Z = (f * base) / d
        if pose is not None:
            T = np.asarray(pose, np.float64)
            X, Y, Z = ((((T[i, 0] * X) + (T[i, 1] * Y)) + (T[i, 2] * Z)) + T[i, 3] for i in range(3))
        out = np.stack([X, Y, Z], axis=-1).astype(np.float32)
    out[~use] = np.nan
    return out


def points_equal(a, b):
    """Bit for bit: the same NaN mask, and the same uint32 words elsewhere."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


# ---- shapes that stress the merge ------------------------------------------------------------------------------------------------
def serpentine(rows, cols, vertical=False, value=320):
    """(map, pixels of the path): a one-pixel path over the whole image: every second row entirely, joined at alternating ends."""
    if vertical:
        m, n = serpentine(cols, rows, False, value)
        return np.ascontiguousarray(m.T), n
    m = np.full((rows, cols), INVALID, np.int16)
    m[0::2, :] = value
    for k, y in enumerate(range(1, rows, 2)):
        if y + 1 < rows:
            m[y, cols - 1 if k % 2 == 0 else 0] = value
    return m, int((m != INVALID).sum())


def spiral(rows, cols, value=320):
    """(map, pixels of the path): a one-pixel spiral from the top left corner inwards, turning right when the way ahead is the
    image's edge or one free pixel before its own earlier arm."""
    m = np.full((rows, cols), INVALID, np.int16)

    def free(y, x, dy, dx):
        ny, nx = y + dy, x + dx
        if not (0 <= ny < rows and 0 <= nx < cols) or m[ny, nx] != INVALID:
            return False
        ay, ax = ny + dy, nx + dx
        return not (0 <= ay < rows and 0 <= ax < cols) or m[ay, ax] == INVALID

    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = value
    while True:
        if not free(y, x, dy, dx):
            dy, dx = dx, -dy
            if not free(y, x, dy, dx):
                break
        y, x = y + dy, x + dx
        m[y, x] = value
    return m, int((m != INVALID).sum())


def comb(rows, cols, value=320):
    """(map, pixels): teeth on every second column over all rows, joined only by the last row."""
    m = np.full((rows, cols), INVALID, np.int16)
    m[:, 0::2] = value
    m[rows - 1, :] = value
    return m, int((m != INVALID).sum())


def corner_crosser(rows, cols, tw, th, value=320):
    """(map, pixels): one component through every tile corner: the two rows and the two columns beside every tile border."""
    m = np.full((rows, cols), INVALID, np.int16)
    for y in range(th, rows, th):
        m[y - 1:y + 1, :] = value
    for x in range(tw, cols, tw):
        m[:, x - 1:x + 1] = value
    if not (m != INVALID).any():
        m[0, 0] = value
    return m, int((m != INVALID).sum())
