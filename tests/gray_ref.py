"""The gray TSDF map of include/viso_hip.h ("TSDF intensity") restated in numpy: the fuse with the image's intensity carried, twice
(vectorised over the pixels, and as a literal per-pixel, per-sample loop into a dict), the sum of gray maps, the intensity of a
vertex, the ray casting with intensity, twice as well, and the bytes of the PLY files with it.  No device and no library.

Rules 1..7 are those of tests/tsdf_ref.py, restated here and not imported, so that "(k, weight, sum) of a gray map equal those of a
plain map" is a check of two texts against each other.  Rule 7 gains: every update of pixel (x, y) also does gray += image[y][x].
Intensity of the point on the edge between voxels a and b (weights wa, wb >= 1, sums of different sign, gray sums ga, gb):
  da = float64(sa) / float64(wa), db likewise, t = da / (da - db); ia = float64(ga) / float64(wa), ib likewise;
  v = ia + (ib - ia) t; g = uint8(min(255.0, floor(v + 0.5))).
Vertex (k, dir): a = k, b = a + (dir & 1, dir >> 1 & 1, dir >> 2); an end that is not in the table, or ends of one sign: 0, missing.
Render: tests/render_ref.py's rules 1..9; the intensity of a valid pixel is g of the hit (a: the previous voxel, b: the hit voxel),
0 where the pixel is INVALID."""
import math

import numpy as np

from map_ref import BIAS, INVALID, RANGE, keys_of, scale
from tsdf_ref import CROSSING, crossing_points, half

ENTRY = np.dtype([("k", np.int32, (3,)), ("weight", np.uint32), ("sum", np.int64), ("gray", np.uint64)])   # struct viso_tsdf_gray_entry, 32 bytes
PLAIN = np.dtype([("k", np.int32, (3,)), ("weight", np.uint32), ("sum", np.int64)])                        # struct viso_tsdf_entry
VERTEX = np.dtype([("k", np.int32, (3,)), ("dir", np.int32), ("p", np.float32, (3,)), ("weight", np.uint32)])


def plain(entries):
    """The (k, weight, sum) of gray entries as a struct viso_tsdf_entry array."""
    e = np.asarray(entries, ENTRY)
    out = np.zeros(len(e), PLAIN)
    out["k"], out["weight"], out["sum"] = e["k"], e["weight"], e["sum"]
    return out


def with_gray(entries, gray):
    """Plain entries and one gray sum per entry as gray entries."""
    e = np.asarray(entries, PLAIN)
    out = np.zeros(len(e), ENTRY)
    out["k"], out["weight"], out["sum"], out["gray"] = e["k"], e["weight"], e["sum"], gray
    return out


def updates(m, image, param, pose, voxel, trunc, min_disp16):
    """(keys [n] int64, q [n] int64, intensity [n] int64 of the updates of step 7, contributing pixels, samples out of range)."""
    m, image = np.asarray(m), np.asarray(image)
    assert m.dtype == np.int16 and m.ndim == 2 and image.dtype == np.uint8 and image.shape == m.shape
    assert min_disp16 >= 1 and 1 <= trunc <= 8
    use = (m != INVALID) & (m >= min_disp16)
    y, x = (a.astype(np.float64) for a in np.nonzero(use))
    pix = image[use].astype(np.int64)
    f, cu, cv, base = (np.float64(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    s, h, lim = scale(voxel), half(voxel), trunc * 1024
    T = None if pose is None else np.asarray(pose, np.float64)
    assert T is None or (T.shape == (4, 4) and np.isfinite(T).all())
    K, Q, G, n_oor = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0
    with np.errstate(all="ignore"):
        d = m[use].astype(np.float64) / 16.0
        X, Y, Z = (base * (x - cu)) / d, (base * (y - cv)) / d, (f * base) / d
        prev = np.full(len(d), -1, np.int64)
        for j in range(-2 * trunc, 2 * trunc + 1):
            zj = Z + np.float64(j) * h
            pos = zj > 0
            r = zj / Z
            Qc = [X * r, Y * r, zj]
            if T is not None:
                Qc = [(((T[i, 0] * Qc[0]) + (T[i, 1] * Qc[1])) + (T[i, 2] * Qc[2])) + T[i, 3] for i in range(3)]
            gd = np.floor(np.stack(Qc, axis=-1) / s)
            inr = (np.abs(gd) < float(RANGE)).all(axis=1)          # False for a NaN
            n_oor += int((pos & ~inr).sum())
            ins = pos & inr
            k = np.where(ins[:, None], gd, 0.0).astype(np.int64) >> 10
            key = keys_of(k)
            C = (k * 1024 + 512).astype(np.float64) * s
            if T is not None:
                zc = ((T[0, 2] * (C[:, 0] - T[0, 3])) + (T[1, 2] * (C[:, 1] - T[1, 3]))) + (T[2, 2] * (C[:, 2] - T[2, 3]))
            else:
                zc = C[:, 2]
            fq = np.floor((Z - zc) / s)
            upd = ins & (key != prev) & (fq >= -lim)               # False for a NaN
            prev = np.where(ins, key, -1)
            K.append(key[upd])
            Q.append(np.minimum(fq[upd], float(lim)).astype(np.int64))
            G.append(pix[upd])
    return np.concatenate(K), np.concatenate(Q), np.concatenate(G), int(use.sum()), n_oor


def _entries(keys, weight, sums, gray):
    out = np.zeros(len(keys), ENTRY)
    out["k"][:, 0] = (keys >> 42) - BIAS
    out["k"][:, 1] = ((keys >> 21) & 0x1FFFFF) - BIAS
    out["k"][:, 2] = (keys & 0x1FFFFF) - BIAS
    out["weight"], out["sum"], out["gray"] = weight, sums, gray
    return out


def _stats(n_points, n_updates, n_oor, n_voxels, capacity_log2):
    return dict(n_points=n_points, n_updates=n_updates, n_out_of_range=n_oor, n_occupied=min(n_voxels, 1 << capacity_log2),
                n_dropped=max(0, n_voxels - (1 << capacity_log2)))


def _accumulate(keys, weights, sums, grays):
    u, inv = np.unique(keys, return_inverse=True)
    w, q, g = (np.zeros(len(u), np.int64) for _ in range(3))
    np.add.at(w, inv, weights)
    np.add.at(q, inv, sums)
    np.add.at(g, inv, grays)
    return _entries(u, w.astype(np.uint32), q, g.astype(np.uint64))


def fuse(frames, param, voxel=0.2, trunc=3, min_disp16=16, capacity_log2=26, min_weight=1):
    """frames: an iterable of (map, image, pose or None).  Returns (gray entries sorted by key, stats); vectorised."""
    K, Q, G, n_points, n_oor = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0, 0
    for m, image, pose in frames:
        k, q, g, n, o = updates(m, image, param, pose, voxel, trunc, min_disp16)
        K.append(k); Q.append(q); G.append(g); n_points += n; n_oor += o
    keys = np.concatenate(K)
    e = _accumulate(keys, np.ones(len(keys), np.int64), np.concatenate(Q), np.concatenate(G))
    return e[e["weight"] >= min_weight], _stats(n_points, len(keys), n_oor, len(e), capacity_log2)


def fuse_loop(frames, param, voxel=0.2, trunc=3, min_disp16=16, capacity_log2=26, min_weight=1):
    """The same, one pixel and one sample at a time into a dict, in Python floats and ints."""
    s, h, lim = float(voxel) / 1024.0, float(voxel) * 0.5, trunc * 1024
    f, cu, cv, base = (float(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    table, n_points, n_updates, n_oor = {}, 0, 0, 0
    for m, image, pose in frames:
        m, image = np.asarray(m), np.asarray(image)
        T = None if pose is None else [[float(v) for v in row] for row in np.asarray(pose, np.float64)]
        for y in range(m.shape[0]):
            for x in range(m.shape[1]):
                d16 = int(m[y, x])
                if d16 == INVALID or d16 < min_disp16:
                    continue
                n_points += 1
                d = d16 / 16.0
                X, Y, Z = base * (x - cu) / d, base * (y - cv) / d, f * base / d
                prev = None
                for j in range(-2 * trunc, 2 * trunc + 1):
                    zj = Z + float(j) * h
                    if not zj > 0:
                        prev = None
                        continue
                    r = zj / Z
                    Q = [X * r, Y * r, zj]
                    if T is not None:
                        Q = [((T[i][0] * Q[0] + T[i][1] * Q[1]) + T[i][2] * Q[2]) + T[i][3] for i in range(3)]
                    quo = [v / s for v in Q]
                    if not all(math.isfinite(v) for v in quo) or any(abs(math.floor(v)) >= RANGE for v in quo):
                        n_oor += 1
                        prev = None
                        continue
                    k = [math.floor(v) >> 10 for v in quo]
                    key = ((k[0] + BIAS) << 42) | ((k[1] + BIAS) << 21) | (k[2] + BIAS)
                    if key == prev:
                        continue
                    prev = key
                    C = [float(v * 1024 + 512) * s for v in k]
                    zc = C[2] if T is None else (T[0][2] * (C[0] - T[0][3]) + T[1][2] * (C[1] - T[1][3])) + T[2][2] * (C[2] - T[2][3])
                    v = (Z - zc) / s
                    if math.isnan(v) or v == -math.inf:
                        continue
                    q = lim if v == math.inf else math.floor(v)
                    if q < -lim:
                        continue
                    rec = table.setdefault(key, [0, 0, 0])
                    rec[0] += 1
                    rec[1] += min(q, lim)
                    rec[2] += int(image[y, x])
                    n_updates += 1
    keys = np.array(sorted(table), np.int64)
    col = [np.array([table[int(k)][i] for k in keys], t) for i, t in enumerate((np.uint32, np.int64, np.uint64))]
    e = _entries(keys, *col)
    return e[e["weight"] >= min_weight], _stats(n_points, n_updates, n_oor, len(keys), capacity_log2)


def merge(*parts):
    """The sum of gray maps given as entry arrays (what viso_tsdf_add_gray_entries does), sorted by key."""
    e = np.concatenate([np.asarray(p, ENTRY) for p in parts]) if parts else np.zeros(0, ENTRY)
    return _accumulate(keys_of(e["k"]), e["weight"].astype(np.int64), e["sum"], e["gray"].astype(np.int64))


def entry_ok(e, trunc):
    """bool [n]: what viso_tsdf_add_gray_entries accepts."""
    e = np.asarray(e, ENTRY)
    w, lim = e["weight"].astype(np.int64), trunc * 1024
    return ((w >= 1) & (np.abs(e["sum"]) <= lim * w) & (e["gray"] <= (255 * w).astype(np.uint64)) &
            (e["k"] >= -BIAS).all(axis=1) & (e["k"] < BIAS).all(axis=1))


# ---- the intensity of a point on an edge -----------------------------------------------------------------------------------------
def edge_gray(wa, sa, ga, wb, sb, gb):
    """uint8 [n], vectorised."""
    wa, wb = np.asarray(wa).astype(np.float64), np.asarray(wb).astype(np.float64)
    da, db = np.asarray(sa).astype(np.float64) / wa, np.asarray(sb).astype(np.float64) / wb
    t = da / (da - db)
    ia, ib = np.asarray(ga).astype(np.float64) / wa, np.asarray(gb).astype(np.float64) / wb
    v = ia + (ib - ia) * t
    return np.minimum(255.0, np.floor(v + 0.5)).astype(np.uint8)


def edge_gray_1(wa, sa, ga, wb, sb, gb):
    """The same for one edge in Python floats."""
    da, db = float(sa) / float(wa), float(sb) / float(wb)
    t = da / (da - db)
    ia, ib = float(ga) / float(wa), float(gb) / float(wb)
    return int(min(255.0, math.floor(ia + (ib - ia) * t + 0.5)))


def vertex_ok(v):
    """bool [n]: the (k, dir) that viso_tsdf_vertex_gray accepts."""
    k, d = np.asarray(v["k"], np.int64), np.asarray(v["dir"], np.int64)
    bit = np.stack([d & 1, (d >> 1) & 1, (d >> 2) & 1], axis=1)
    return (d >= 1) & (d <= 7) & (k >= -BIAS).all(axis=1) & (k < BIAS - bit).all(axis=1)


def crossing_vertices(c):
    """The crossings of tsdf_ref.crossings as (k, dir = 1 << axis)."""
    c = np.asarray(c, CROSSING)
    v = np.zeros(len(c), VERTEX)
    v["k"], v["dir"] = c["k"], 1 << c["axis"]
    return v


def vertex_gray(entries, vertices):
    """(uint8 [n], number missing) of gray entries sorted by key and a (k, dir) list that vertex_ok accepts."""
    e = np.asarray(entries, ENTRY)
    keys = keys_of(e["k"])
    assert (np.diff(keys) > 0).all() and vertex_ok(vertices).all()
    out = np.zeros(len(vertices), np.uint8)
    if not len(e) or not len(vertices):
        return out, len(vertices)
    d = vertices["dir"].astype(np.int64)
    ka = vertices["k"].astype(np.int64)
    kb = ka + np.stack([d & 1, (d >> 1) & 1, d >> 2], axis=1)
    a, b = (np.minimum(np.searchsorted(keys, keys_of(k)), len(keys) - 1) for k in (ka, kb))
    ok = (keys[a] == keys_of(ka)) & (keys[b] == keys_of(kb)) & ((e["sum"][a] < 0) != (e["sum"][b] < 0))
    a, b = a[ok], b[ok]
    out[ok] = edge_gray(e["weight"][a], e["sum"][a], e["gray"][a], e["weight"][b], e["sum"][b], e["gray"][b])
    return out, int((~ok).sum())


# ---- ray casting with intensity --------------------------------------------------------------------------------------------------
def n_samples(voxel, max_depth):
    n = int(np.floor(np.float64(max_depth) / half(voxel)))
    assert 1 <= n <= 65536
    return n


def _centre_depth(k, s, T):
    C = (k * 1024 + 512).astype(np.float64) * s
    if T is None:
        return C[:, 2]
    return ((T[0, 2] * (C[:, 0] - T[0, 3])) + (T[1, 2] * (C[:, 1] - T[1, 3]))) + (T[2, 2] * (C[:, 2] - T[2, 3]))


def render(entries, voxel, param, shape, pose=None, max_depth=40.0, min_weight=2):
    """(disp16 int16, weight uint32, gray uint8, each [rows][cols]); vectorised over the pixels, a loop over the samples."""
    e = np.asarray(entries, ENTRY)
    keys = keys_of(e["k"])
    assert (np.diff(keys) > 0).all() and min_weight >= 1
    rows, cols = shape
    f, cu, cv, base = (np.float64(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    s, h, N = scale(voxel), half(voxel), n_samples(voxel, max_depth)
    T = None if pose is None else np.asarray(pose, np.float64)
    assert T is None or (T.shape == (4, 4) and np.isfinite(T).all())
    y, x = (v.reshape(-1).astype(np.float64) for v in np.mgrid[0:rows, 0:cols])
    out_d = np.full(rows * cols, INVALID, np.int16)
    out_w = np.zeros(rows * cols, np.uint32)
    out_g = np.zeros(rows * cols, np.uint8)
    at = np.arange(rows * cols)
    a, b = (x - cu) / f, (y - cv) / f
    pk = np.zeros((len(at), 3), np.int64)
    pkey = np.full(len(at), -1, np.int64)
    pw, ps, pg = (np.zeros(len(at), np.int64) for _ in range(3))
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
            pkey[~inr], pw[~inr] = -1, 0                           # a gap
            new = np.nonzero(inr & (key != pkey))[0]
            if not len(new):
                continue
            if len(keys):
                pos = np.minimum(np.searchsorted(keys, key[new]), len(keys) - 1)
                found = keys[pos] == key[new]
                w = np.where(found, e["weight"][pos].astype(np.int64), 0)
                sm = np.where(found, e["sum"][pos], 0)
                gs = np.where(found, e["gray"][pos].astype(np.int64), 0)
            else:
                w, sm, gs = (np.zeros(len(new), np.int64) for _ in range(3))
            w = np.where(w >= min_weight, w, 0)
            hit = (w > 0) & (sm < 0) & (pw[new] > 0) & (ps[new] >= 0)
            hn = new[hit]
            if len(hn):
                za, zb = _centre_depth(pk[hn], s, T), _centre_depth(k[hn], s, T)
                da = ps[hn].astype(np.float64) / pw[hn].astype(np.float64)
                db = sm[hit].astype(np.float64) / w[hit].astype(np.float64)
                t = da / (da - db)
                zs = za + (zb - za) * t
                v = ((f * base) / zs) * 16.0 + 0.5
                ok = (zs > 0) & (v >= 1.0) & ~(v >= 32768.0)
                out_d[at[hn[ok]]] = np.floor(v[ok]).astype(np.int16)
                out_w[at[hn[ok]]] = np.minimum(pw[hn], w[hit])[ok].astype(np.uint32)
                out_g[at[hn[ok]]] = edge_gray(pw[hn], ps[hn], pg[hn], w[hit], sm[hit], gs[hit])[ok]
            on = new[~hit]
            pk[on], pkey[on], pw[on], ps[on], pg[on] = k[on], key[on], w[~hit], sm[~hit], gs[~hit]
            if len(hn):
                keep = np.ones(len(at), bool)
                keep[hn] = False
                at, a, b, pk, pkey, pw, ps, pg = at[keep], a[keep], b[keep], pk[keep], pkey[keep], pw[keep], ps[keep], pg[keep]
    return out_d.reshape(rows, cols), out_w.reshape(rows, cols), out_g.reshape(rows, cols)


def render_loop(entries, voxel, param, shape, pose=None, max_depth=40.0, min_weight=2):
    """The same, one pixel and one sample at a time, in Python floats and ints over a dict."""
    e = np.asarray(entries, ENTRY)
    table = {int(key): (int(w), int(q), int(g)) for key, w, q, g in zip(keys_of(e["k"]), e["weight"], e["sum"], e["gray"])}
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
    out_g = np.zeros((rows, cols), np.uint8)
    for y in range(rows):
        for x in range(cols):
            a, b = (float(x) - cu) / f, (float(y) - cv) / f
            prev = None                                            # (key, k, weight or 0, sum, gray)
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
                w, q, g = table.get(key, (0, 0, 0))
                if w < min_weight:
                    w = 0
                if w and q < 0 and prev is not None and prev[2] and prev[3] >= 0:
                    za, zb = depth(prev[1]), depth(k)
                    da, db = float(prev[3]) / float(prev[2]), float(q) / float(w)
                    t = da / (da - db)
                    zs = za + (zb - za) * t
                    v = ((f * base) / zs) * 16.0 + 0.5 if zs != 0.0 else math.nan
                    if zs > 0 and v >= 1.0 and not v >= 32768.0:
                        out_d[y, x] = math.floor(v)
                        out_w[y, x] = min(prev[2], w)
                        out_g[y, x] = edge_gray_1(prev[2], prev[3], prev[4], w, q, g)
                    break
                prev = (key, k, w, q, g)
    return out_d, out_w, out_g


# ---- the PLY files with intensity ------------------------------------------------------------------------------------------------
_RGB = "property uchar red\nproperty uchar green\nproperty uchar blue\n"


def mesh_ply_bytes(vertices, triangles, gray):
    """The PLY file of write_mesh_ply(..., gray): per vertex x, y, z float32, weight uint32 and red = green = blue = gray as uchar;
    per face one uchar 3 and three int32 indices."""
    v = np.asarray(vertices, VERTEX)
    tri = np.asarray(triangles, np.uint32).reshape(-1, 3)
    head = ("ply\nformat binary_little_endian 1.0\ncomment libviso_amd TSDF mesh\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\nproperty uint weight\n%selement face %d\n"
            "property list uchar int vertex_indices\nend_header\n" % (len(v), _RGB, len(tri)))
    body = b"".join(v["p"][i].astype("<f4").tobytes() + v["weight"][i].astype("<u4").tobytes() + bytes([int(gray[i])] * 3)
                    for i in range(len(v)))
    faces = b"".join(b"\x03" + tri[i].astype("<i4").tobytes() for i in range(len(tri)))
    return head.encode("ascii") + body + faces


def surface_ply_bytes(c, voxel, gray):
    """The PLY file of write_surface_ply(..., gray): x, y, z the float32 crossing points, weight = min(wa, wb), then the three
    equal uchar."""
    c = np.asarray(c, CROSSING)
    p = crossing_points(c, voxel)
    head = ("ply\nformat binary_little_endian 1.0\ncomment libviso_amd TSDF surface, voxel %r m\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\nproperty uint weight\n%send_header\n" % (float(voxel), len(c), _RGB))
    body = b"".join(p[i].astype("<f4").tobytes() + np.uint32(min(c["wa"][i], c["wb"][i])).astype("<u4").tobytes() +
                    bytes([int(gray[i])] * 3) for i in range(len(c)))
    return head.encode("ascii") + body
