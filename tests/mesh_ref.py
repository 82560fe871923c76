"""The triangle mesh of a TSDF map (include/viso_hip.h, "TSDF mesh") restated in numpy from the geometric rule, without a table of
cases: the triangles of a tetrahedron are worked out from its four signs by the rule itself (tet_triangles), once per tetrahedron
and sign pattern that occurs, and applied to all cells with that pattern at once.  Also the bytes of the PLY file.

  Usable: weight >= min_weight.  Negative: sum < 0.  The cell of voxel k: corners k + (dx, dy, dz), all eight usable, no k_i = 2^20 - 1.
  Tetrahedra: the permutations pi of (0, 1, 2) in lexicographic order; c0 = k, c1 = c0 + e_pi0, c2 = c1 + e_pi1, c3 = k + (1, 1, 1).
  Edge (ci, cj), i < j: owner ci, d = cj - ci, dir = dx + 2 dy + 4 dz.  It carries a vertex when the signs of its ends differ:
  t = da / (da - db) with the means da = sa / wa, db = sb / wb, p_i = float32((float64(a_i 1024 + 512) + (t 1024 if d_i else 0)) s).
  One corner i alone on its side: (e(i, j1), e(i, j2), e(i, j3)), j ascending.  N = {a, b}, P = {c, d}: (e(a, c), e(a, d), e(b, d)) and
  (e(a, c), e(b, d), e(b, c)).  With every vertex at its edge midpoint (2 owner + d in half voxels), n = (v1 - v0) x (v2 - v0) and
  g = |N| sum_P c - |P| sum_N c: v1 and v2 are swapped when n . g < 0.
  Vertices: those some triangle refers to, sorted by (key of owner, dir).  Triangles: sorted by (key of cell, tetrahedron, index)."""
import functools
import itertools

import numpy as np

from map_ref import BIAS, keys_of, scale
from tsdf_ref import ENTRY

VERTEX = np.dtype([("k", np.int32, (3,)), ("dir", np.int32), ("p", np.float32, (3,)), ("weight", np.uint32)])   # viso_tsdf_mesh_vertex, 32 bytes
PERMS = list(itertools.permutations(range(3)))          # lexicographic


def tet_corners(tet):
    """The four corners of tetrahedron `tet` of a cell as offsets from the cell's voxel, int [4][3]."""
    c = np.zeros((4, 3), np.int64)
    for i, axis in enumerate(PERMS[tet]):
        c[i + 1] = c[i]
        c[i + 1, axis] += 1
    return c


def code(d):
    return int(d[0] + 2 * d[1] + 4 * d[2])


@functools.lru_cache(maxsize=None)
def tet_triangles(tet, neg):
    """The rule for one tetrahedron: neg is a tuple of four bools (corner i negative).  A list of triangles, each three pairs
    (corner offset code of the edge's owner, dir), oriented."""
    c = tet_corners(tet)
    N = [i for i in range(4) if neg[i]]
    P = [i for i in range(4) if not neg[i]]
    if not N or not P:
        return []
    if len(N) == 1 or len(P) == 1:
        i = N[0] if len(N) == 1 else P[0]
        tris = [[(i, j) for j in range(4) if j != i]]
    else:
        (a, b), (cc, d) = N, P
        tris = [[(a, cc), (a, d), (b, d)], [(a, cc), (b, d), (b, cc)]]
    g = len(N) * c[P].sum(axis=0) - len(P) * c[N].sum(axis=0)
    out = []
    for tri in tris:
        e = [(min(i, j), max(i, j)) for i, j in tri]
        mid = [c[i] + c[j] for i, j in e]                # 2 owner + d
        n = np.cross(mid[1] - mid[0], mid[2] - mid[0])
        s = int(n @ g)
        assert s != 0
        if s < 0:
            e[1], e[2] = e[2], e[1]
        out.append([(code(c[i]), code(c[j] - c[i])) for i, j in e])
    return out


def _neighbours(e, keys):
    """idx [8][n]: the position in e of voxel + (dx, dy, dz) for the corner codes 0..7, or -1."""
    n = len(e)
    idx = np.full((8, n), -1, np.int64)
    idx[0] = np.arange(n)
    for c in range(1, 8):
        d = np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], np.int64)
        ok = ((e["k"] < BIAS - 1) | (d == 0)).all(axis=1)          # no key is formed beyond a field
        want = keys + ((d[0] << 42) + (d[1] << 21) + d[2])
        at = np.minimum(np.searchsorted(keys, want), max(n - 1, 0))
        hit = ok & (keys[at] == want) if n else np.zeros(0, bool)
        idx[c] = np.where(hit, at, -1)
    return idx


def mesh(entries, voxel, min_weight=1):
    """(vertices VERTEX [nv], triangles uint32 [nt][3]) of an entry array sorted by key."""
    e = np.asarray(entries, ENTRY)
    e = e[e["weight"] >= min_weight]
    keys = keys_of(e["k"])
    assert (np.diff(keys) > 0).all()
    idx = _neighbours(e, keys)
    cells = np.nonzero((idx >= 0).all(axis=0))[0]
    neg = e["sum"][idx[:, cells]] < 0 if len(cells) else np.zeros((8, 0), bool)      # [8][cells]
    T = []                                                                          # rows: cell, tet, index, 3 x vertex id
    for tet in range(6):
        cc = [code(c) for c in tet_corners(tet)]
        pat = sum(neg[cc[i]].astype(np.int64) << i for i in range(4))
        for p in range(1, 15):
            sel = np.nonzero(pat == p)[0]
            if not len(sel):
                continue
            for q, tri in enumerate(tet_triangles(tet, tuple(bool(p >> i & 1) for i in range(4)))):
                row = np.zeros((len(sel), 6), np.int64)
                row[:, 0], row[:, 1], row[:, 2] = cells[sel], tet, q
                for m, (corner, d) in enumerate(tri):
                    row[:, 3 + m] = idx[corner, cells[sel]] * 8 + d                 # vertex id: (owner, dir)
                T.append(row)
    T = np.concatenate(T) if T else np.zeros((0, 6), np.int64)
    T = T[np.lexsort((T[:, 2], T[:, 1], T[:, 0]))]
    ids = np.unique(T[:, 3:])
    tri = np.searchsorted(ids, T[:, 3:]).astype(np.uint32).reshape(-1, 3)
    a, d = ids >> 3, ids & 7
    b = idx[d, a]
    assert (b >= 0).all() and ((e["sum"][a] < 0) != (e["sum"][b] < 0)).all()
    v = np.zeros(len(ids), VERTEX)
    v["k"], v["dir"], v["weight"] = e["k"][a], d, np.minimum(e["weight"][a], e["weight"][b])
    da = e["sum"][a].astype(np.float64) / e["weight"][a].astype(np.float64)
    db = e["sum"][b].astype(np.float64) / e["weight"][b].astype(np.float64)
    t = da / (da - db)
    centre = (e["k"][a].astype(np.int64) * 1024 + 512).astype(np.float64)
    on = np.stack([d & 1, (d >> 1) & 1, (d >> 2) & 1], axis=1) != 0
    v["p"] = ((centre + np.where(on, (t * 1024.0)[:, None], 0.0)) * scale(voxel)).astype(np.float32)
    return v, tri


def midpoints2(v):
    """The edge midpoints of a vertex array in half voxels: 2 owner + d, int64 [n][3]."""
    d = v["dir"].astype(np.int64)
    return 2 * v["k"].astype(np.int64) + np.stack([d & 1, (d >> 1) & 1, (d >> 2) & 1], axis=1)


def ply_bytes(vertices, triangles):
    """The PLY file of write_mesh_ply: binary little-endian; per vertex x, y, z float32 and weight uint32; per face one uchar 3 and
    three int32 indices."""
    v = np.asarray(vertices, VERTEX)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3)
    head = ("ply\nformat binary_little_endian 1.0\ncomment libviso_amd TSDF mesh\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\nproperty uint weight\nelement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(v), len(tri)))
    body = b"".join(v["p"][i].astype("<f4").tobytes() + v["weight"][i].astype("<u4").tobytes() for i in range(len(v)))
    faces = b"".join(b"\x03" + tri[i].astype("<i4").tobytes() for i in range(len(tri)))
    return head.encode("ascii") + body + faces


def sphere_entries(n=12, centre=5.3, radius=3.7, trunc=3, weight=1):
    """The voxels 0 .. n-1 cubed, sorted by key, with the distance of the index from (centre, centre, centre) less the radius, in
    units of 1 / 1024 voxel, floored and clamped to trunc 1024, times the weight: negative inside the sphere."""
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    d = np.sqrt(((g - centre) ** 2).sum(axis=1)) - radius
    e = np.zeros(len(g), ENTRY)
    e["k"], e["weight"] = g, weight
    e["sum"] = np.clip(np.floor(d * 1024.0), -trunc * 1024, trunc * 1024).astype(np.int64) * weight
    return e[np.argsort(keys_of(e["k"]))]


def closed_and_oriented(tri):
    """(every directed edge occurs once and its reverse once, number of undirected edges)."""
    t = np.asarray(tri, np.int64).reshape(-1, 3)
    de = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    code = de[:, 0] * (int(t.max()) + 1 if len(t) else 1) + de[:, 1]
    back = de[:, 1] * (int(t.max()) + 1 if len(t) else 1) + de[:, 0]
    once = len(np.unique(code)) == len(code)
    return bool(once and np.array_equal(np.sort(code), np.sort(back))), len(code) // 2
