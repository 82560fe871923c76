"""The TSDF map of include/viso_hip.h ("TSDF map") restated in numpy, twice: vectorised over the pixels (np.unique over the keys,
np.add.at) and as a literal per-pixel, per-sample loop into a dict.  Also the surface crossings, their points, the sum of maps and
the bytes of the PLY file.

Parameters: voxel > 0 and finite, trunc_voxels T in 1..8, min_disp16 >= 1, capacity_log2 in 10..28; s = voxel / 1024 and
h = voxel * 0.5 in double.  Everything is IEEE double in the operand order written, no fused multiply-add.
  1. A pixel (x, y) contributes when disp16 != INVALID and disp16 >= min_disp16.
  2. d = disp16 / 16, X = base (x - cu) / d, Y = base (y - cv) / d, Z = f base / d.
  3. For j = -2T .. 2T ascending: zj = Z + float64(j) h.  !(zj > 0): not inserted, resets rule 5.  r = zj / Z, Qc = (X r, Y r, zj),
     Q_i = ((T[i][0] Qc0 + T[i][1] Qc1) + T[i][2] Qc2) + T[i][3]; no pose: Q = Qc.
  4. g_i = floor(Q_i / s).  Any |g_i| >= 2^30 or not finite: not inserted, n_out_of_range += 1, resets rule 5.  k_i = g_i >> 10.
  5. A sample whose voxel equals that of the pixel's previous inserted sample is skipped.
  6. C_i = float64(k_i 1024 + 512) s, zc = (T[0][2] (C0 - T[0][3]) + T[1][2] (C1 - T[1][3])) + T[2][2] (C2 - T[2][3]) (no pose: C2),
     q = floor((Z - zc) / s).  !(q >= -T 1024): no update (the sample still is rule 5's previous one).  q > T 1024: q = T 1024.
  7. weight += 1, sum += q.
  8. Entries with weight >= min_weight, sorted by key.
  9. For every such voxel a and axis 0, 1, 2: b = a + e_axis; when b is such a voxel too and (sum_a < 0) != (sum_b < 0), a crossing
     (k, axis, wa, wb, sa, sb).  Sorted by (key of a, axis).
 10. da = float64(sa) / float64(wa), db likewise, t = da / (da - db),
     p_i = float32((float64(k_i 1024 + 512) + (t 1024 if i == axis else 0)) s)."""
import math

import numpy as np

from map_ref import BIAS, INVALID, RANGE, keys_of, scale

ENTRY = np.dtype([("k", np.int32, (3,)), ("weight", np.uint32), ("sum", np.int64)])                      # struct viso_tsdf_entry, 24 bytes
CROSSING = np.dtype([("k", np.int32, (3,)), ("axis", np.int32), ("wa", np.uint32), ("wb", np.uint32), ("sa", np.int64),
                     ("sb", np.int64)])                                                                 # struct viso_tsdf_crossing, 40 bytes


def half(voxel):
    return np.float64(voxel) * np.float64(0.5)


def updates(m, param, pose, voxel, trunc, min_disp16):
    """(keys [n] int64, q [n] int64 of the updates of step 7, number of contributing pixels, number of samples out of range)."""
    m = np.asarray(m)
    assert m.dtype == np.int16 and m.ndim == 2 and min_disp16 >= 1 and 1 <= trunc <= 8
    use = (m != INVALID) & (m >= min_disp16)
    y, x = (a.astype(np.float64) for a in np.nonzero(use))
    f, cu, cv, base = (np.float64(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    s, h, lim = scale(voxel), half(voxel), trunc * 1024
    T = None if pose is None else np.asarray(pose, np.float64)
    assert T is None or (T.shape == (4, 4) and np.isfinite(T).all())
    K, Q, n_oor = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0
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
    return np.concatenate(K), np.concatenate(Q), int(use.sum()), n_oor


def _entries(keys, weight, sums):
    out = np.zeros(len(keys), ENTRY)
    out["k"][:, 0] = (keys >> 42) - BIAS
    out["k"][:, 1] = ((keys >> 21) & 0x1FFFFF) - BIAS
    out["k"][:, 2] = (keys & 0x1FFFFF) - BIAS
    out["weight"], out["sum"] = weight, sums
    return out


def _stats(n_points, n_updates, n_oor, n_voxels, capacity_log2):
    """n_dropped: 0 when the voxels fit the table; otherwise at least one update per voxel beyond it is dropped."""
    return dict(n_points=n_points, n_updates=n_updates, n_out_of_range=n_oor, n_occupied=min(n_voxels, 1 << capacity_log2),
                n_dropped=max(0, n_voxels - (1 << capacity_log2)))


def _accumulate(keys, weights, sums):
    u, inv = np.unique(keys, return_inverse=True)
    w = np.zeros(len(u), np.int64)
    q = np.zeros(len(u), np.int64)
    np.add.at(w, inv, weights)
    np.add.at(q, inv, sums)
    return _entries(u, w.astype(np.uint32), q)


def fuse(frames, param, voxel=0.2, trunc=3, min_disp16=16, capacity_log2=26, min_weight=1):
    """frames: an iterable of (map, pose or None).  Returns (entries sorted by key, stats); vectorised."""
    K, Q, n_points, n_oor = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0, 0
    for m, pose in frames:
        k, q, n, o = updates(m, param, pose, voxel, trunc, min_disp16)
        K.append(k); Q.append(q); n_points += n; n_oor += o
    keys, q = np.concatenate(K), np.concatenate(Q)
    e = _accumulate(keys, np.ones(len(keys), np.int64), q)
    return e[e["weight"] >= min_weight], _stats(n_points, len(keys), n_oor, len(e), capacity_log2)


def fuse_loop(frames, param, voxel=0.2, trunc=3, min_disp16=16, capacity_log2=26, min_weight=1):
    """The same, one pixel and one sample at a time into a dict, in Python floats and ints."""
    s, h, lim = float(voxel) / 1024.0, float(voxel) * 0.5, trunc * 1024
    f, cu, cv, base = (float(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    table, n_points, n_updates, n_oor = {}, 0, 0, 0
    for m, pose in frames:
        m = np.asarray(m)
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
                    rec = table.setdefault(key, [0, 0])
                    rec[0] += 1
                    rec[1] += min(q, lim)
                    n_updates += 1
    keys = np.array(sorted(table), np.int64)
    e = _entries(keys, np.array([table[int(k)][0] for k in keys], np.uint32), np.array([table[int(k)][1] for k in keys], np.int64))
    return e[e["weight"] >= min_weight], _stats(n_points, n_updates, n_oor, len(keys), capacity_log2)


def merge(*parts):
    """The sum of maps given as entry arrays (what viso_tsdf_add_entries does), sorted by key."""
    e = np.concatenate([np.asarray(p, ENTRY) for p in parts]) if parts else np.zeros(0, ENTRY)
    return _accumulate(keys_of(e["k"]), e["weight"].astype(np.int64), e["sum"])


def crossings(entries, min_weight=1):
    """Step 9 over an entry array sorted by key."""
    e = np.asarray(entries, ENTRY)
    e = e[e["weight"] >= min_weight]
    keys = keys_of(e["k"])
    assert (np.diff(keys) > 0).all()
    parts = []
    for axis in range(3):
        a = np.nonzero(e["k"][:, axis] < BIAS - 1)[0]                  # the last voxel of an axis has no neighbour
        want = keys[a] + (1 << (21 * (2 - axis)))
        b = np.minimum(np.searchsorted(keys, want), max(len(keys) - 1, 0))
        hit = (keys[b] == want) & ((e["sum"][a] < 0) != (e["sum"][b] < 0)) if len(keys) else np.zeros(0, bool)
        a, b = a[hit], b[hit]
        c = np.zeros(len(a), CROSSING)
        c["k"], c["axis"], c["wa"], c["wb"], c["sa"], c["sb"] = e["k"][a], axis, e["weight"][a], e["weight"][b], e["sum"][a], e["sum"][b]
        parts.append(c)
    c = np.concatenate(parts)
    return c[np.lexsort((c["axis"], keys_of(c["k"])))]


def crossing_points(c, voxel):
    """float32 [n][3]: step 10."""
    c = np.asarray(c, CROSSING)
    da = c["sa"].astype(np.float64) / c["wa"].astype(np.float64)
    db = c["sb"].astype(np.float64) / c["wb"].astype(np.float64)
    t = da / (da - db)
    centre = (c["k"].astype(np.int64) * 1024 + 512).astype(np.float64)
    off = np.zeros((len(c), 3))
    off[np.arange(len(c)), c["axis"]] = t * 1024.0
    return ((centre + off) * scale(voxel)).astype(np.float32)


def ply_bytes(c, voxel):
    """The PLY file of write_surface_ply: binary little-endian, x, y, z the float32 crossing points and weight = min(wa, wb) as
    uint32, in the crossings' order."""
    c = np.asarray(c, CROSSING)
    p = crossing_points(c, voxel)
    head = ("ply\nformat binary_little_endian 1.0\ncomment libviso_amd TSDF surface, voxel %r m\nelement vertex %d\n"
            "property float x\nproperty float y\nproperty float z\nproperty uint weight\nend_header\n" % (float(voxel), len(c)))
    body = b"".join(p[i].astype("<f4").tobytes() + np.uint32(min(c["wa"][i], c["wb"][i])).astype("<u4").tobytes() for i in range(len(c)))
    return head.encode("ascii") + body
