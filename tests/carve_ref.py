"""The TSDF map with fuse options (include/viso_hip.h, "TSDF fuse options": free-space carving and disparity-based weights) restated
in numpy, twice: vectorised over the pixels, and as a literal per-pixel, per-sample loop into a dict.  Plain and gray maps.  No
device and no library.

Rules 1..7 are those of tests/tsdf_ref.py and tests/gray_ref.py, restated here and not imported (only the packing of the entry
arrays and of the statistics is theirs), so that "default options give tsdf_ref.fuse byte for byte" is a check of two texts
against each other.  What the options change:
  3. j runs over -(2T + 2C) .. 2T ascending.  A sample with j < -2T is a free-space sample; one with zj < carve_near is not inserted
     and resets rule 5, like !(zj > 0).  Rules 4, 5, 6 apply to free-space samples unchanged.
  7. w = 1 when weight_shift is None (the C struct: < 0), else w = min(max((disp16 disp16) >> weight_shift, 1), weight_max) in
     integers, with the pixel's own disp16.  weight += w, sum += w q, gray += w I.  n_updates counts updates, not weights.
Both forms assert that no voxel's weight reaches 2^32."""
import math

import numpy as np

import gray_ref
import tsdf_ref
from map_ref import BIAS, INVALID, RANGE, keys_of, scale
from tsdf_ref import half

DEFAULTS = dict(carve_voxels=0, weight_shift=None, weight_max=255, carve_near=0.0)


def _options(opts):
    o = dict(DEFAULTS, **opts)
    assert set(o) == set(DEFAULTS) and 0 <= o["carve_voxels"] <= 1024 and math.isfinite(o["carve_near"]) and o["carve_near"] >= 0
    assert o["weight_shift"] is None or (0 <= o["weight_shift"] <= 30 and 1 <= o["weight_max"] <= 255)
    return o["carve_voxels"], o["weight_shift"], o["weight_max"], float(o["carve_near"])


def weight_of(d16, weight_shift=None, weight_max=255):
    """Rule 7's w of one pixel, in Python integers."""
    if weight_shift is None:
        return 1
    return min(max((int(d16) * int(d16)) >> weight_shift, 1), weight_max)


def weights_of(d16, weight_shift=None, weight_max=255):
    """The same of an array, int64 (disp16 < 2^15: the square fits the uint32 of the definition)."""
    d = np.asarray(d16).astype(np.int64)
    if weight_shift is None:
        return np.ones(d.shape, np.int64)
    return np.minimum(np.maximum((d * d) >> weight_shift, 1), weight_max)


def updates(m, image, param, pose, voxel, trunc, min_disp16, **opts):
    """(keys, q, w, intensity: [n] int64 each, of the updates of step 7; contributing pixels; samples out of range).  image None:
    the intensities are zeros."""
    carve, shift, wmax, near = _options(opts)
    m = np.asarray(m)
    assert m.dtype == np.int16 and m.ndim == 2 and min_disp16 >= 1 and 1 <= trunc <= 8
    use = (m != INVALID) & (m >= min_disp16)
    if image is None:
        pix = np.zeros(int(use.sum()), np.int64)
    else:
        image = np.asarray(image)
        assert image.dtype == np.uint8 and image.shape == m.shape
        pix = image[use].astype(np.int64)
    y, x = (a.astype(np.float64) for a in np.nonzero(use))
    f, cu, cv, base = (np.float64(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    s, h, lim = scale(voxel), half(voxel), trunc * 1024
    T = None if pose is None else np.asarray(pose, np.float64)
    assert T is None or (T.shape == (4, 4) and np.isfinite(T).all())
    w = weights_of(m[use], shift, wmax)
    K, Q, W, G, n_oor = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0
    with np.errstate(all="ignore"):
        d = m[use].astype(np.float64) / 16.0
        X, Y, Z = (base * (x - cu)) / d, (base * (y - cv)) / d, (f * base) / d
        prev = np.full(len(d), -1, np.int64)
        for j in range(-(2 * trunc + 2 * carve), 2 * trunc + 1):
            zj = Z + np.float64(j) * h
            pos = zj > 0
            if j < -2 * trunc:
                pos &= ~(zj < near)
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
            W.append(w[upd])
            G.append(pix[upd])
    return np.concatenate(K), np.concatenate(Q), np.concatenate(W), np.concatenate(G), int(use.sum()), n_oor


def _entries(keys, weight, sums, grays, gray):
    assert (np.asarray(weight, np.int64) < 2 ** 32).all(), "a voxel's weight has reached 2^32"
    if gray:
        return gray_ref._entries(keys, np.asarray(weight).astype(np.uint32), sums, np.asarray(grays).astype(np.uint64))
    return tsdf_ref._entries(keys, np.asarray(weight).astype(np.uint32), sums)


def _frames(frames, gray):
    """(map, image or None, pose) of every frame: a gray map's frames are (map, image, pose), a plain one's (map, pose)."""
    for fr in frames:
        yield fr if gray else (fr[0], None, fr[1])


def fuse(frames, param, voxel=0.2, trunc=3, min_disp16=16, capacity_log2=26, min_weight=1, gray=False, **opts):
    """frames: an iterable of (map, pose or None), with gray of (map, image, pose or None).  Returns (entries sorted by key:
    tsdf_ref.ENTRY, with gray gray_ref.ENTRY; stats); vectorised."""
    K, Q, W, G, n_points, n_oor = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0, 0
    for m, image, pose in _frames(frames, gray):
        k, q, w, g, n, o = updates(m, image, param, pose, voxel, trunc, min_disp16, **opts)
        K.append(k); Q.append(q); W.append(w); G.append(g); n_points += n; n_oor += o
    keys, q, w, g = (np.concatenate(v) for v in (K, Q, W, G))
    u, inv = np.unique(keys, return_inverse=True)
    sw, sq, sg = (np.zeros(len(u), np.int64) for _ in range(3))
    np.add.at(sw, inv, w)
    np.add.at(sq, inv, w * q)
    np.add.at(sg, inv, w * g)
    e = _entries(u, sw, sq, sg, gray)
    return e[e["weight"] >= min_weight], tsdf_ref._stats(n_points, len(keys), n_oor, len(e), capacity_log2)


def samples(d16, x, y, param, pose, voxel, trunc, **opts):
    """Every sample of one pixel, literally: a list of (j, voxel (kx, ky, kz) or None when the sample is not inserted, q or None when
    it makes no update, w), j ascending.  Out-of-range samples are listed as (j, "oor", None, w)."""
    carve, shift, wmax, near = _options(opts)
    s, h, lim = float(voxel) / 1024.0, float(voxel) * 0.5, trunc * 1024
    f, cu, cv, base = (float(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    T = None if pose is None else [[float(v) for v in row] for row in np.asarray(pose, np.float64)]
    w = weight_of(d16, shift, wmax)
    d = int(d16) / 16.0
    X, Y, Z = base * (x - cu) / d, base * (y - cv) / d, f * base / d
    out, prev = [], None
    for j in range(-(2 * trunc + 2 * carve), 2 * trunc + 1):
        zj = Z + float(j) * h
        if not zj > 0 or (j < -2 * trunc and zj < near):
            prev = None
            out.append((j, None, None, w))
            continue
        r = zj / Z if Z != 0.0 else math.nan
        Q = [X * r, Y * r, zj]
        if T is not None:
            Q = [((T[i][0] * Q[0] + T[i][1] * Q[1]) + T[i][2] * Q[2]) + T[i][3] for i in range(3)]
        quo = [v / s for v in Q]
        if not all(math.isfinite(v) for v in quo) or any(abs(math.floor(v)) >= RANGE for v in quo):
            prev = None
            out.append((j, "oor", None, w))
            continue
        k = tuple(math.floor(v) >> 10 for v in quo)
        if k == prev:
            continue                                               # rule 5: not a sample of its own
        prev = k
        C = [float(v * 1024 + 512) * s for v in k]
        zc = C[2] if T is None else (T[0][2] * (C[0] - T[0][3]) + T[1][2] * (C[1] - T[1][3])) + T[2][2] * (C[2] - T[2][3])
        v = (Z - zc) / s
        q = None
        if not (math.isnan(v) or v == -math.inf):
            q = lim if v == math.inf else math.floor(v)
            q = None if q < -lim else min(q, lim)
        out.append((j, k, q, w))
    return out


def fuse_loop(frames, param, voxel=0.2, trunc=3, min_disp16=16, capacity_log2=26, min_weight=1, gray=False, **opts):
    """The same as fuse, one pixel and one sample at a time into a dict, in Python floats and ints."""
    table, n_points, n_updates, n_oor = {}, 0, 0, 0
    for m, image, pose in _frames(frames, gray):
        m = np.asarray(m)
        for y in range(m.shape[0]):
            for x in range(m.shape[1]):
                d16 = int(m[y, x])
                if d16 == INVALID or d16 < min_disp16:
                    continue
                n_points += 1
                for _, k, q, w in samples(d16, x, y, param, pose, voxel, trunc, **opts):
                    if k == "oor":
                        n_oor += 1
                    if k is None or k == "oor" or q is None:
                        continue
                    key = ((k[0] + BIAS) << 42) | ((k[1] + BIAS) << 21) | (k[2] + BIAS)
                    rec = table.setdefault(key, [0, 0, 0])
                    rec[0] += w
                    rec[1] += w * q
                    rec[2] += w * (int(image[y, x]) if image is not None else 0)
                    n_updates += 1
    keys = np.array(sorted(table), np.int64)
    col = [np.array([table[int(k)][i] for k in keys], np.int64) for i in range(3)]
    e = _entries(keys, *col, gray)
    return e[e["weight"] >= min_weight], tsdf_ref._stats(n_points, n_updates, n_oor, len(keys), capacity_log2)
