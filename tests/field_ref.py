"""The distance field of include/viso_hip.h ("TSDF distance field") restated in numpy: usable voxels and their states from a dict of
keys, surface voxels by looking up the six neighbours, and the distances by brute force over the list of sites, in chunks.  No
separable passes: a mistake in the device's three passes cannot be shared with this file.

  1. Box: n = hi - lo in 1..512 an axis; cell (i0, i1, i2) is the voxel lo + i, at index (i0 n1 + i1) n2 + i2.
  2. Usable: every k_i in -2^20 .. 2^20 - 1, in the table, weight >= min_weight >= 1.
  3. State: 0 unknown, 1 front (sum >= 0), 2 behind (sum < 0).
  4. Surface voxel: usable with a usable neighbour k + e or k - e on some axis whose (sum < 0) differs; the neighbour may be outside
     the box; the first and the last index of an axis have no neighbour on that side.  State |= SURFACE.
  5. Sites: the surface voxels of the box; with UNKNOWN_IS_SITE the unknown cells too.
  6. sq[c] = min over sites of the squared distance in cells, NONE when the box holds no site.

No device and no library at module level."""
import numpy as np

BIAS = 1 << 20
UNKNOWN_IS_SITE = 1
SURFACE = 4
NONE = 0xffffffff
MAX_AXIS = 512


def shape_of(box):
    lo, hi = (np.asarray(v).astype(np.int64) for v in box)
    n = hi - lo
    assert lo.shape == hi.shape == (3,) and (n >= 1).all() and (n <= MAX_AXIS).all(), n
    return lo, tuple(int(v) for v in n)


def states(entries, min_weight, box):
    """uint8 [n0][n1][n2]: rules 2 to 4 for every cell of the box.  entries: sorted by key, any entry dtype with k, weight, sum."""
    assert min_weight >= 1
    lo, n = shape_of(box)
    table = {}
    for k, w, s in zip(entries["k"].tolist(), entries["weight"].tolist(), entries["sum"].tolist()):
        if w >= min_weight:                          # usable voxels only: the others are unknown to every rule
            table[tuple(k)] = s < 0
    assert len(table) == int((entries["weight"] >= min_weight).sum())     # no key twice
    st = np.zeros(n, np.uint8)
    hi = lo + np.asarray(n)
    for k, neg in table.items():
        if not all(lo[i] <= k[i] < hi[i] for i in range(3)):
            continue
        assert all(-BIAS <= v < BIAS for v in k)
        v = 2 if neg else 1
        for ax in range(3):
            for step in (1, -1):
                if not -BIAS <= k[ax] + step < BIAS:     # nothing beyond the key range, and nothing wraps
                    continue
                nb = table.get(tuple(k[i] + (step if i == ax else 0) for i in range(3)))
                if nb is not None and nb != neg:
                    v |= SURFACE
        st[k[0] - lo[0], k[1] - lo[1], k[2] - lo[2]] = v
    return st


def sites_of(st, flags=0):
    """bool [n0][n1][n2]: rule 5."""
    assert flags & ~UNKNOWN_IS_SITE == 0
    site = (st & SURFACE) != 0
    if flags & UNKNOWN_IS_SITE:
        site |= st == 0
    return site


def brute_loop(site):
    """brute, literally: (c - s)^2 summed over the axes in int64, one cell at a time.  For small boxes."""
    s = np.argwhere(site).astype(np.int64)
    out = np.full(site.shape, NONE, np.uint32)
    if len(s):
        for c in np.ndindex(*site.shape):
            d = np.asarray(c, np.int64) - s
            out[c] = (d * d).sum(axis=1).min()
    return out


def brute(site, chunk=1 << 24):
    """uint32, the shape of `site`: rule 6 by brute force, every cell against every site of the list, `chunk` pairs at a time.
    |c - s|^2 = |c|^2 + (|s|^2 - 2 c . s), the bracket as one product of [c, 1] with [-2 s, |s|^2] in float32: every term and
    every partial sum is an integer below 9 * 511^2 < 2^24, so the arithmetic is exact in any order."""
    n = site.shape
    assert max(n) <= MAX_AXIS
    s = np.argwhere(site).astype(np.int64)
    if not len(s):
        return np.full(n, NONE, np.uint32)
    cells = np.stack(np.meshgrid(*[np.arange(v, dtype=np.int64) for v in n], indexing="ij"), axis=-1).reshape(-1, 3)
    left = np.concatenate([cells, np.ones((len(cells), 1), np.int64)], axis=1).astype(np.float32)
    right = np.concatenate([-2 * s, (s * s).sum(axis=1, keepdims=True)], axis=1).astype(np.float32).T.copy()
    out = np.empty(len(cells), np.int64)
    step = max(1, chunk // len(s))
    for a in range(0, len(cells), step):
        out[a:a + step] = (left[a:a + step] @ right).min(axis=1).astype(np.int64)
    out += (cells * cells).sum(axis=1)
    assert out.min() >= 0 and out.max() <= 3 * (MAX_AXIS - 1) ** 2
    return out.astype(np.uint32).reshape(n)


def field(entries, min_weight, box, flags=0):
    """(sq uint32 [n0][n1][n2], state uint8 of that shape, n_sites) of viso_tsdf_distance_field."""
    st = states(entries, min_weight, box)
    site = sites_of(st, flags)
    return brute(site), st, int(site.sum())
