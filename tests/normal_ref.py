"""The surface normals of include/viso_hip.h ("TSDF normals") restated in numpy, twice: vectorised over the items (the keys looked
up in the sorted entry array by searchsorted) and as a literal loop per item in Python floats and ints over a dict, which can count
the branches of the rule it met.  Their input is the entry array of tests/tsdf_ref.py, so neither needs a device.  The vertices
are tests/mesh_ref.py's and tests/tsdf_ref.py's crossings; the hits of a render are found by the march of tests/render_ref.py,
restated here with the two voxels of every hit kept, and held to render_ref.render's disparities and weights.

IEEE double in the operand order written.
  Usable voxel: in the table with weight >= min_weight >= 1; d(v) = float64(sum_v) / float64(weight_v).
  Gradient of a usable voxel v, per axis i with p = v + e_i, m = v - e_i (an index that would leave the key range: not usable):
    both usable G_i = (d(p) - d(m)) * 0.5; only p: d(p) - d(v); only m: d(v) - d(m); neither: v has no gradient.
  Normal on the edge (a, b): a, b usable with (sa < 0) != (sb < 0), else missing; t = da / (da - db); both ends need a gradient,
    else missing; g_i = Ga_i + (Gb_i - Ga_i) t; L = sqrt((g0 g0 + g1 g1) + g2 g2); !(L > 0) or not finite: missing;
    n_i = g_i / L; the output is float32(n_i), a missing normal (0, 0, 0).
  Vertex (k, dir): a = k, b = a + (dir & 1, dir >> 1 & 1, dir >> 2), in the world frame.
  Render: a the previous voxel of render_ref's rule 6, b the hit voxel, only at a valid pixel; with a pose T the normal goes into
    the camera frame before the cast, nc_j = (T[0][j] n0 + T[1][j] n1) + T[2][j] n2; no pose: nc = n."""
import math

import numpy as np

import render_ref as RR
from map_ref import BIAS, INVALID, RANGE, keys_of, scale
from mesh_ref import VERTEX
from tsdf_ref import CROSSING, ENTRY, half

# what the loop form counts: per axis of a gradient central / up_only / down_only / no_gradient; per edge same_sign (usable ends of
# one sign), end_absent (an end that is not usable), zero_length (!(L > 0) or not finite), normal (a normal came out)
BRANCHES = ("central", "up_only", "down_only", "no_gradient", "same_sign", "end_absent", "zero_length", "normal")


def vertex_ok(v):
    """bool [n]: the (k, dir) that viso_tsdf_vertex_normals accepts."""
    k, d = np.asarray(v["k"], np.int64), np.asarray(v["dir"], np.int64)
    bit = np.stack([d & 1, (d >> 1) & 1, (d >> 2) & 1], axis=1)
    return (d >= 1) & (d <= 7) & (k >= -BIAS).all(axis=1) & (k < BIAS - bit).all(axis=1)


def crossing_vertices(c):
    """The crossings of tsdf_ref.crossings as (k, dir = 1 << axis)."""
    c = np.asarray(c, CROSSING)
    v = np.zeros(len(c), VERTEX)
    v["k"], v["dir"] = c["k"], 1 << c["axis"]
    return v


def edge_ends(vertices):
    """(ka, kb) int64 [n][3] of a (k, dir) list."""
    d = vertices["dir"].astype(np.int64)
    ka = vertices["k"].astype(np.int64)
    return ka, ka + np.stack([d & 1, (d >> 1) & 1, d >> 2], axis=1)


# ---- vectorised ------------------------------------------------------------------------------------------------------------------
class _Usable:
    """The usable voxels of an entry array sorted by key: find(k) -> (found bool [n], d float64 [n], sum int64 [n])."""

    def __init__(self, entries, min_weight):
        e = np.asarray(entries, ENTRY)
        assert min_weight >= 1 and (np.diff(keys_of(e["k"])) > 0).all()
        e = e[e["weight"] >= min_weight]
        self.keys, self.sum = keys_of(e["k"]), e["sum"]
        self.d = e["sum"].astype(np.float64) / e["weight"].astype(np.float64)

    def find(self, k):
        k = np.asarray(k, np.int64)
        inside = ((k >= -BIAS) & (k < BIAS)).all(axis=1)           # an index beyond the key range: not usable
        if not len(self.keys):
            return np.zeros(len(k), bool), np.zeros(len(k)), np.zeros(len(k), np.int64)
        key = keys_of(np.where(inside[:, None], k, 0))
        at = np.minimum(np.searchsorted(self.keys, key), len(self.keys) - 1)
        found = inside & (self.keys[at] == key)
        return found, np.where(found, self.d[at], 0.0), np.where(found, self.sum[at], 0)


def gradients(u, k, d):
    """(has bool [n], G float64 [n][3]) of the usable voxels k of distance d."""
    G, has = np.zeros((len(k), 3)), np.ones(len(k), bool)
    for i in range(3):
        step = np.zeros(3, np.int64)
        step[i] = 1
        up, dp, _ = u.find(k + step)
        down, dm, _ = u.find(k - step)
        G[:, i] = np.where(up & down, (dp - dm) * 0.5, np.where(up, dp - d, d - dm))
        has &= up | down
    return has, G


def edge_normals(entries, min_weight, ka, kb):
    """(n float64 [n][3] in the world frame, ok bool [n]) of the edges between the voxels ka and kb; rows without a normal are 0."""
    u = _Usable(entries, min_weight)
    ka, kb = np.asarray(ka, np.int64).reshape(-1, 3), np.asarray(kb, np.int64).reshape(-1, 3)
    fa, da, sa = u.find(ka)
    fb, db, sb = u.find(kb)
    ok = fa & fb & ((sa < 0) != (sb < 0))
    ha, Ga = gradients(u, ka, da)
    hb, Gb = gradients(u, kb, db)
    ok &= ha & hb
    with np.errstate(all="ignore"):
        t = da / (da - db)
        g = Ga + (Gb - Ga) * t[:, None]
        L = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        ok &= (L > 0) & np.isfinite(L)
        n = g / L[:, None]
    return np.where(ok[:, None], n, 0.0), ok


def vertex_normals(entries, vertices, min_weight=1):
    """(float32 [n][3], number missing) of an entry array sorted by key and a (k, dir) list that vertex_ok accepts."""
    assert vertex_ok(vertices).all()
    n, ok = edge_normals(entries, min_weight, *edge_ends(vertices))
    return n.astype(np.float32), int((~ok).sum())


def rotate(n, pose):
    """World normals float64 [..][3] into the camera frame of pose (None: as they are)."""
    if pose is None:
        return n
    T = np.asarray(pose, np.float64)
    return np.stack([(T[0, j] * n[..., 0] + T[1, j] * n[..., 1]) + T[2, j] * n[..., 2] for j in range(3)], axis=-1)


def hits(entries, voxel, param, shape, pose=None, max_depth=40.0, min_weight=2):
    """(disp16 int16 [rows][cols], weight uint32 [rows][cols], ka, kb int64 [rows][cols][3]): render_ref.render's march with the two
    voxels of every valid hit kept (0 elsewhere).  The first two are asserted to be render_ref.render's."""
    e = np.asarray(entries, ENTRY)
    keys = keys_of(e["k"])
    assert (np.diff(keys) > 0).all() and min_weight >= 1
    rows, cols = shape
    f, cu, cv, base = RR._calib(param)
    s, h, N = scale(voxel), half(voxel), RR.n_samples(voxel, max_depth)
    T = None if pose is None else np.asarray(pose, np.float64)
    y, x = (v.reshape(-1).astype(np.float64) for v in np.mgrid[0:rows, 0:cols])
    out_d = np.full(rows * cols, INVALID, np.int16)
    out_w = np.zeros(rows * cols, np.uint32)
    out_a, out_b = np.zeros((rows * cols, 3), np.int64), np.zeros((rows * cols, 3), np.int64)
    at = np.arange(rows * cols)
    a, b = (x - cu) / f, (y - cv) / f
    pk = np.zeros((len(at), 3), np.int64)
    pkey = np.full(len(at), -1, np.int64)
    pw, ps = np.zeros(len(at), np.int64), np.zeros(len(at), np.int64)
    with np.errstate(all="ignore"):
        for i in range(1, N + 1):
            if not len(at):
                break
            z = np.float64(i) * h
            Q = [a * z, b * z, np.full(len(at), z)]
            if T is not None:
                Q = [(((T[r, 0] * Q[0]) + (T[r, 1] * Q[1])) + (T[r, 2] * Q[2])) + T[r, 3] for r in range(3)]
            gd = [np.floor(q / s) for q in Q]
            inr = (np.abs(gd[0]) < float(RANGE)) & (np.abs(gd[1]) < float(RANGE)) & (np.abs(gd[2]) < float(RANGE))
            gd = [np.where(inr, g, 0.0) for g in gd]
            k = np.stack([g.astype(np.int64) >> 10 for g in gd], axis=-1)
            key = keys_of(k)
            pkey[~inr], pw[~inr] = -1, 0
            new = np.nonzero(inr & (key != pkey))[0]
            if not len(new):
                continue
            if len(keys):
                pos = np.minimum(np.searchsorted(keys, key[new]), len(keys) - 1)
                found = keys[pos] == key[new]
                w = np.where(found, e["weight"][pos].astype(np.int64), 0)
                sm = np.where(found, e["sum"][pos], 0)
            else:
                w, sm = np.zeros(len(new), np.int64), np.zeros(len(new), np.int64)
            w = np.where(w >= min_weight, w, 0)
            hit = (w > 0) & (sm < 0) & (pw[new] > 0) & (ps[new] >= 0)
            hn = new[hit]
            if len(hn):
                za, zb = RR._centre_depth(pk[hn], s, T), RR._centre_depth(k[hn], s, T)
                da = ps[hn].astype(np.float64) / pw[hn].astype(np.float64)
                db = sm[hit].astype(np.float64) / w[hit].astype(np.float64)
                t = da / (da - db)
                zs = za + (zb - za) * t
                v = ((f * base) / zs) * 16.0 + 0.5
                ok = (zs > 0) & (v >= 1.0) & ~(v >= 32768.0)
                to = at[hn[ok]]
                out_d[to] = np.floor(v[ok]).astype(np.int16)
                out_w[to] = np.minimum(pw[hn], w[hit])[ok].astype(np.uint32)
                out_a[to], out_b[to] = pk[hn[ok]], k[hn[ok]]
            on = new[~hit]
            pk[on], pkey[on], pw[on], ps[on] = k[on], key[on], w[~hit], sm[~hit]
            if len(hn):
                keep = np.ones(len(at), bool)
                keep[hn] = False
                at, a, b, pk, pkey, pw, ps = at[keep], a[keep], b[keep], pk[keep], pkey[keep], pw[keep], ps[keep]
    d, w = out_d.reshape(rows, cols), out_w.reshape(rows, cols)
    want = RR.render(entries, voxel, param, shape, pose, max_depth, min_weight)
    assert d.tobytes() == want[0].tobytes() and w.tobytes() == want[1].tobytes()
    return d, w, out_a.reshape(rows, cols, 3), out_b.reshape(rows, cols, 3)


def render_world(entries, voxel, param, shape, pose=None, max_depth=40.0, min_weight=2):
    """(disp16, weight, world normals float64 [rows][cols][3], has a normal bool [rows][cols])."""
    d, w, ka, kb = hits(entries, voxel, param, shape, pose, max_depth, min_weight)
    n, ok = edge_normals(entries, min_weight, ka.reshape(-1, 3), kb.reshape(-1, 3))
    ok &= (d != INVALID).reshape(-1)
    return d, w, np.where(ok[:, None], n, 0.0).reshape(shape + (3,)), ok.reshape(shape)


def render(entries, voxel, param, shape, pose=None, max_depth=40.0, min_weight=2):
    """(disp16 int16, weight uint32, normals float32 [rows][cols][3] in the camera frame of pose); vectorised."""
    d, w, n, _ = render_world(entries, voxel, param, shape, pose, max_depth, min_weight)
    return d, w, rotate(n, pose).astype(np.float32)


# ---- one item at a time ----------------------------------------------------------------------------------------------------------
def _table(entries):
    e = np.asarray(entries, ENTRY)
    return {int(key): (int(w), int(q)) for key, w, q in zip(keys_of(e["k"]), e["weight"], e["sum"])}


def _usable_1(table, min_weight, k):
    """(weight, sum) of the usable voxel k, or None."""
    if any(v < -BIAS or v >= BIAS for v in k):
        return None
    rec = table.get(((k[0] + BIAS) << 42) | ((k[1] + BIAS) << 21) | (k[2] + BIAS))
    return rec if rec is not None and rec[0] >= min_weight else None


def _gradient_1(table, min_weight, k, d, trace):
    G = []
    for i in range(3):
        p, m = ([v + (j == i) * sgn for j, v in enumerate(k)] for sgn in (1, -1))
        rp, rm = _usable_1(table, min_weight, p), _usable_1(table, min_weight, m)
        dp, dm = (None if r is None else float(r[1]) / float(r[0]) for r in (rp, rm))
        if rp and rm:
            branch, g = "central", (dp - dm) * 0.5
        elif rp:
            branch, g = "up_only", dp - d
        elif rm:
            branch, g = "down_only", d - dm
        else:
            branch, g = "no_gradient", None
        if trace is not None:
            trace[branch] += 1
        G.append(g)
    return None if any(g is None for g in G) else G


def edge_normal_1(table, min_weight, ka, kb, trace=None):
    """The normal [3] in Python floats of the edge between ka and kb in the world frame, or None: missing."""
    ra, rb = _usable_1(table, min_weight, ka), _usable_1(table, min_weight, kb)
    if ra is None or rb is None:
        if trace is not None:
            trace["end_absent"] += 1
        return None
    if (ra[1] < 0) == (rb[1] < 0):
        if trace is not None:
            trace["same_sign"] += 1
        return None
    da, db = float(ra[1]) / float(ra[0]), float(rb[1]) / float(rb[0])
    t = da / (da - db)
    Ga, Gb = _gradient_1(table, min_weight, ka, da, trace), _gradient_1(table, min_weight, kb, db, trace)
    if Ga is None or Gb is None:
        return None
    g = [Ga[i] + (Gb[i] - Ga[i]) * t for i in range(3)]
    L = math.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    if not L > 0 or not math.isfinite(L):
        if trace is not None:
            trace["zero_length"] += 1
        return None
    if trace is not None:
        trace["normal"] += 1
    return [v / L for v in g]


def vertex_normals_loop(entries, vertices, min_weight=1, trace=None):
    """vertex_normals, one vertex at a time; trace: a collections.Counter of BRANCHES, on which the results do not depend."""
    assert vertex_ok(vertices).all()
    table = _table(entries)
    out, missing = np.zeros((len(vertices), 3), np.float32), 0
    for i in range(len(vertices)):
        ka, d = [int(v) for v in vertices["k"][i]], int(vertices["dir"][i])
        n = edge_normal_1(table, min_weight, ka, [ka[0] + (d & 1), ka[1] + (d >> 1 & 1), ka[2] + (d >> 2)], trace)
        if n is None:
            missing += 1
        else:
            out[i] = n
    return out, missing


def render_loop(entries, voxel, param, shape, pose=None, max_depth=40.0, min_weight=2, trace=None):
    """render, one pixel and one sample at a time (render_ref.render_loop's march, with the hit's voxels kept)."""
    table = _table(entries)
    rows, cols = shape
    f, cu, cv, base = (float(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    s, h = float(voxel) / 1024.0, float(voxel) * 0.5
    N = int(math.floor(float(max_depth) / h))
    assert 1 <= N <= 65536 and min_weight >= 1
    T = None if pose is None else [[float(v) for v in row] for row in np.asarray(pose, np.float64)]

    def depth(k):
        C = [float(v * 1024 + 512) * s for v in k]
        return C[2] if T is None else (T[0][2] * (C[0] - T[0][3]) + T[1][2] * (C[1] - T[1][3])) + T[2][2] * (C[2] - T[2][3])

    out_d = np.full((rows, cols), INVALID, np.int16)
    out_w = np.zeros((rows, cols), np.uint32)
    out_n = np.zeros((rows, cols, 3), np.float32)
    for y in range(rows):
        for x in range(cols):
            a, b = (float(x) - cu) / f, (float(y) - cv) / f
            prev = None                                            # (key, k, weight or 0, sum)
            for i in range(1, N + 1):
                z = float(i) * h
                Q = [a * z, b * z, z]
                if T is not None:
                    Q = [((T[r][0] * Q[0] + T[r][1] * Q[1]) + T[r][2] * Q[2]) + T[r][3] for r in range(3)]
                quo = [v / s for v in Q]
                if not all(math.isfinite(v) for v in quo) or any(abs(math.floor(v)) >= RANGE for v in quo):
                    prev = None
                    continue
                k = [math.floor(v) >> 10 for v in quo]
                key = ((k[0] + BIAS) << 42) | ((k[1] + BIAS) << 21) | (k[2] + BIAS)
                if prev is not None and key == prev[0]:
                    continue
                w, q = table.get(key, (0, 0))
                if w < min_weight:
                    w = 0
                if w and q < 0 and prev is not None and prev[2] and prev[3] >= 0:
                    za, zb = depth(prev[1]), depth(k)
                    da, db = float(prev[3]) / float(prev[2]), float(q) / float(w)
                    try:
                        t = da / (da - db)
                        zs = za + (zb - za) * t
                        v = ((f * base) / zs) * 16.0 + 0.5
                    except ZeroDivisionError:
                        zs = v = math.nan
                    if zs > 0 and v >= 1.0 and not v >= 32768.0:
                        out_d[y, x] = math.floor(v)
                        out_w[y, x] = min(prev[2], w)
                        n = edge_normal_1(table, min_weight, prev[1], k, trace)
                        if n is not None:
                            out_n[y, x] = n if T is None else [(T[0][j] * n[0] + T[1][j] * n[1]) + T[2][j] * n[2] for j in range(3)]
                    break
                prev = (key, k, w, q)
    return out_d, out_w, out_n


# ---- views smaller than the fused maps ---------------------------------------------------------------------------------------------
def window(param, shape, full_shape, hole=0.0, inside=20):
    """The calibration of a view of `shape` that is a window of the maps of full_shape that `param` belongs to: the principal point
    moved with the window's corner.  A map fused from a view of three rows or of one pixel is one voxel thick and has no gradient,
    so the small views of the normals' tests look at maps fused from full_shape.  The window lies about the middle row; with more
    than one column it ends `inside` columns inside the columns that render_ref.scene_map(.., full_shape, hole) leaves invalid, so
    that a view from the fusing pose has valid and invalid pixels."""
    from libviso_amd.abi import Param
    rows, cols = shape
    if tuple(shape) == tuple(full_shape):
        return Param.default(base=param.base, f=param.f, cu=param.cu, cv=param.cv)
    invalid_from = full_shape[1] - (max(1, int(full_shape[1] * hole)) if hole else 0)
    col0 = invalid_from + inside - cols if cols > 1 else full_shape[1] // 3
    row0 = (full_shape[0] - rows) // 2
    assert 0 <= col0 and col0 + cols <= full_shape[1] and 0 <= row0
    return Param.default(base=param.base, f=param.f, cu=param.cu - col0, cv=param.cv - row0)


# ---- a table for the branch that no random block meets ---------------------------------------------------------------------------
def flat_table():
    """(entries, vertices): the voxel a at the origin with sum 0 and its upper x neighbour b below zero, so t = 0 and g = Ga; a's
    lower x neighbour has b's distance and its four other neighbours share one, so Ga = (0, 0, 0) and L = 0: the edge (a, 1) has
    usable ends of different sign with gradients and still no normal.  The edge (b, 1) beside it has one."""
    k = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (2, 0, 0), (1, 1, 0), (1, 0, 1), (2, 1, 0), (2, 0, 1)]
    sums = [0, -10, -10, 14, 14, 14, 14, 40, 6, 6, 8, 8]
    e = np.zeros(len(k), ENTRY)
    e["k"], e["weight"], e["sum"] = k, 2, sums
    v = np.zeros(2, VERTEX)
    v["k"], v["dir"] = [(0, 0, 0), (1, 0, 0)], 1
    return e[np.argsort(keys_of(e["k"]))], v
