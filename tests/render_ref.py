"""The ray casting of include/viso_hip.h ("TSDF render") restated in numpy, twice: vectorised over the pixels (a loop over the
samples, the keys looked up in the sorted entry array by searchsorted) and as a literal loop per pixel and per sample in Python
floats and ints over a dict.  Their input is the entry array of tests/tsdf_ref.py, so neither needs a device.  Also the scenes the
render tests share (a wall, a slanted plane, a depth step) with the disparity a perfect renderer would give for them.

Inputs: min_weight >= 1, the calibration f, cu, cv, base, (rows, cols), max_depth > 0, a pose (4 x 4, camera to world) or None.
s = voxel / 1024, h = voxel * 0.5, N = int(floor(max_depth / h)) in 1 .. 65536.  IEEE double in the operand order written.
  1. a = (float64(x) - cu) / f, b = (float64(y) - cv) / f.
  2. For i = 1 .. N ascending: z = float64(i) h, Qc = (a z, b z, z), Q_i = ((T[i][0] Qc0 + T[i][1] Qc1) + T[i][2] Qc2) + T[i][3]
     (no pose: Q = Qc).
  3. g_i = floor(Q_i / s), k_i = g_i >> 10.  Any |g_i| >= 2^30 or not finite: the sample is a gap.
  4. A sample whose voxel equals that of the previous non-gap sample is skipped; a gap empties "previous".
  5. A voxel is usable when it is in the table with weight >= min_weight; one that is not still becomes "previous", not usable.
  6. Hit: the first sample whose voxel b is usable with sum_b < 0 and whose previous voxel a is usable with sum_a >= 0.
  7. C_i = float64(k_i 1024 + 512) s, zc = (T[0][2] (C0 - T[0][3]) + T[1][2] (C1 - T[1][3])) + T[2][2] (C2 - T[2][3]) (no pose: C2)
     for a and b; da = float64(sa) / float64(wa), db likewise, t = da / (da - db), zs = za + (zb - za) t.
  8. v = ((f base) / zs) 16 + 0.5.  !(zs > 0), !(v >= 1) or v >= 32768: invalid.  Else disp16 = floor(v), weight = min(wa, wb).
  9. No hit or an invalid value: INVALID, weight 0."""
import math

import numpy as np

from map_ref import BIAS, INVALID, RANGE, keys_of, scale
from tsdf_ref import ENTRY, half


def n_samples(voxel, max_depth):
    n = int(np.floor(np.float64(max_depth) / half(voxel)))
    assert 1 <= n <= 65536
    return n


def _calib(param):
    return tuple(np.float64(getattr(param, k)) for k in ("f", "cu", "cv", "base"))


def _centre_depth(k, s, T):
    C = (k * 1024 + 512).astype(np.float64) * s
    if T is None:
        return C[:, 2]
    return ((T[0, 2] * (C[:, 0] - T[0, 3])) + (T[1, 2] * (C[:, 1] - T[1, 3]))) + (T[2, 2] * (C[:, 2] - T[2, 3]))


def render(entries, voxel, param, shape, pose=None, max_depth=40.0, min_weight=2):
    """(disp16 int16 [rows][cols], weight uint32 [rows][cols]); vectorised.  entries: sorted by key (tsdf_ref.fuse)."""
    e = np.asarray(entries, ENTRY)
    keys = keys_of(e["k"])
    assert (np.diff(keys) > 0).all() and min_weight >= 1
    rows, cols = shape
    f, cu, cv, base = _calib(param)
    s, h, N = scale(voxel), half(voxel), n_samples(voxel, max_depth)
    T = None if pose is None else np.asarray(pose, np.float64)
    assert T is None or (T.shape == (4, 4) and np.isfinite(T).all())
    y, x = (v.reshape(-1).astype(np.float64) for v in np.mgrid[0:rows, 0:cols])
    out_d = np.full(rows * cols, INVALID, np.int16)
    out_w = np.zeros(rows * cols, np.uint32)
    # the pixels still marching, and per such pixel the previous voxel of its sequence (key -1: none; weight 0: not usable)
    at = np.arange(rows * cols)
    a, b = (x - cu) / f, (y - cv) / f
    pk = np.zeros((len(at), 3), np.int64)
    pkey = np.full(len(at), -1, np.int64)
    pw = np.zeros(len(at), np.int64)
    ps = np.zeros(len(at), np.int64)
    with np.errstate(all="ignore"):
        for i in range(1, N + 1):
            if not len(at):
                break
            z = np.float64(i) * h
            Q = [a * z, b * z, np.full(len(at), z)]
            if T is not None:
                Q = [(((T[r, 0] * Q[0]) + (T[r, 1] * Q[1])) + (T[r, 2] * Q[2])) + T[r, 3] for r in range(3)]
            gd = [np.floor(q / s) for q in Q]
            inr = (np.abs(gd[0]) < float(RANGE)) & (np.abs(gd[1]) < float(RANGE)) & (np.abs(gd[2]) < float(RANGE))   # False for a NaN
            if not inr.all():
                gd = [np.where(inr, g, 0.0) for g in gd]
            k = np.stack([g.astype(np.int64) >> 10 for g in gd], axis=-1)
            key = ((k[:, 0] + BIAS) << 42) | ((k[:, 1] + BIAS) << 21) | (k[:, 2] + BIAS)
            if not inr.all():
                pkey[~inr], pw[~inr] = -1, 0                       # a gap
            new = np.nonzero(inr & (key != pkey))[0]
            if not len(new):
                continue
            pos = np.minimum(np.searchsorted(keys, key[new]), max(len(keys) - 1, 0))
            found = keys[pos] == key[new] if len(keys) else np.zeros(len(new), bool)
            w = np.where(found, e["weight"][pos].astype(np.int64), 0) if len(keys) else np.zeros(len(new), np.int64)
            sm = np.where(found, e["sum"][pos], 0) if len(keys) else np.zeros(len(new), np.int64)
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
            on = new[~hit]
            pk[on], pkey[on], pw[on], ps[on] = k[on], key[on], w[~hit], sm[~hit]
            if len(hn):
                keep = np.ones(len(at), bool)
                keep[hn] = False
                at, a, b, pk, pkey, pw, ps = at[keep], a[keep], b[keep], pk[keep], pkey[keep], pw[keep], ps[keep]
    return out_d.reshape(rows, cols), out_w.reshape(rows, cols)


EVENTS = ("gap", "first_negative", "negative_after_unusable", "negative_after_negative", "backface", "front_sum_zero",
          "zero_after_positive", "underweight", "hit", "hit_too_big", "hit_too_small", "hit_behind")


def render_loop(entries, voxel, param, shape, pose=None, max_depth=40.0, min_weight=2, trace=None):
    """The same, one pixel and one sample at a time, in Python floats and ints over a dict.

    trace: a collections.Counter that counts, over all pixels, what the rule met (EVENTS); the results do not depend on it.
    Per sample: gap (step 3, also where a whole ray is gaps).  Per voxel entered (step 4): underweight (in the table, below
    min_weight); for a usable voxel with sum < 0: first_negative (no previous voxel), negative_after_unusable (the previous voxel is
    absent or underweight), negative_after_negative, or hit; for a usable voxel with sum >= 0 after a usable one: backface (the
    previous sum < 0) or, with sum == 0, zero_after_positive (the previous sum >= 0: no hit, only sum < 0 is behind the surface).
    Per hit: front_sum_zero (sum_a == 0), and of an invalid value (step 8) hit_behind (!(zs > 0)), else hit_too_big (v >= 32768),
    else hit_too_small (!(v >= 1))."""
    e = np.asarray(entries, ENTRY)
    table = {int(key): (int(w), int(q)) for key, w, q in zip(keys_of(e["k"]), e["weight"], e["sum"])}
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
                    if trace is not None:
                        trace["gap"] += 1
                    continue
                k = [math.floor(v) >> 10 for v in quo]
                key = ((k[0] + BIAS) << 42) | ((k[1] + BIAS) << 21) | (k[2] + BIAS)
                if prev is not None and key == prev[0]:
                    continue
                w, q = table.get(key, (0, 0))
                if w < min_weight:
                    if trace is not None and w:
                        trace["underweight"] += 1
                    w = 0
                if trace is not None and w:
                    _trace_voxel(trace, q, prev)
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
                    elif trace is not None:
                        trace["hit_behind" if not zs > 0 else "hit_too_big" if v >= 32768.0 else "hit_too_small"] += 1
                    break
                prev = (key, k, w, q)
    return out_d, out_w


def _trace_voxel(trace, q, prev):
    """The event of a usable voxel of sum q that follows prev (None, or (key, k, weight or 0, sum)) in a ray's sequence."""
    if q < 0:
        if prev is None:
            trace["first_negative"] += 1
        elif not prev[2]:
            trace["negative_after_unusable"] += 1
        elif prev[3] < 0:
            trace["negative_after_negative"] += 1
        else:
            trace["hit"] += 1
            if prev[3] == 0:
                trace["front_sum_zero"] += 1
    elif prev is not None and prev[2]:
        if prev[3] < 0:
            trace["backface"] += 1
        elif q == 0:
            trace["zero_after_positive"] += 1


# ---- the scenes of the render tests: maps a camera at the fusing pose measures, and what a perfect renderer gives elsewhere ----------
SCENES = ("wall", "plane", "step")


def _parts(name, cols):
    """The scene as pieces (disparity at the middle column in px, px a column, first column, end column)."""
    return {"wall": [(40.0, 0.0, 0, cols)], "plane": [(40.0, 0.03, 0, cols)],
            "step": [(40.0, 0.0, 0, cols // 2), (25.0, 0.0, cols // 2, cols)]}[name]


def scene_map(name, shape, hole=0.0):
    """int16 [rows][cols].  wall: fronto-parallel, constant disparity 640 = 40 px.  plane: slanted about the vertical axis, 40 px at
    the middle column and 0.03 px more a column (a plane of space is an affine function of the pixel in disparity).  step: the left
    half at 40 px, the right half at 25 px.  hole: this part of the columns, at the right, is INVALID (at least one column)."""
    rows, cols = shape
    x = np.arange(cols, dtype=np.float64)
    d = np.zeros(cols)
    for p, g, x0, x1 in _parts(name, cols):
        d[x0:x1] = (p + g * (x - (cols - 1) / 2.0))[x0:x1]
    m = np.repeat(np.floor(d * 16.0 + 0.5).astype(np.int16)[None], rows, axis=0)
    if hole:
        m[:, cols - max(1, int(cols * hole)):] = INVALID
    return m


def ideal(name, shape, param, fuse_pose, view_pose, fused_shape=None, hole=0.0):
    """float64 [rows][cols]: the disparity in px a perfect renderer at view_pose gives for the surface that a camera at fuse_pose
    measured as scene_map(name, fused_shape, hole), NaN where its ray meets none of it.  The surface exists only where a pixel of
    the fused map saw it.  Rays are (a, b, 1), so the ray parameter is the depth along the view's own z axis."""
    fused_shape = fused_shape or shape
    frows, fcols = fused_shape
    f, cu, cv, base = _calib(param)
    Tf = np.eye(4) if fuse_pose is None else np.asarray(fuse_pose, np.float64)
    Tv = np.eye(4) if view_pose is None else np.asarray(view_pose, np.float64)
    y, x = np.mgrid[0:shape[0], 0:shape[1]].astype(np.float64)
    d = np.stack([(x - cu) / f, (y - cv) / f, np.ones(shape)], axis=-1) @ Tv[:3, :3].T
    # into the fusing camera's coordinates, where a piece is d(x) = p + g (x - xm): the plane f base = Z (p - g xm) + g (f X + cu Z)
    Ri = Tf[:3, :3].T
    o, d = Ri @ (Tv[:3, 3] - Tf[:3, 3]), d @ Ri.T
    xm = (fcols - 1) / 2.0
    end = fcols - max(1, int(fcols * hole)) if hole else fcols
    best = np.full(shape, np.inf)
    with np.errstate(all="ignore"):
        for p, g, x0, x1 in _parts(name, fcols):
            n = np.array([g * f, 0.0, p - g * xm + g * cu])
            t = (f * base - n @ o) / (d @ n)
            P = o + d * t[..., None]
            xf, yf = f * P[..., 0] / P[..., 2] + cu, f * P[..., 1] / P[..., 2] + cv
            seen = (t > 0) & (P[..., 2] > 0) & (xf >= x0 - 0.5) & (xf < min(x1, end) - 0.5) & (yf >= -0.5) & (yf < frows - 0.5)
            best = np.where(seen & (t < best), t, best)
    return np.where(np.isfinite(best), (f * base) / best, np.nan)


def sideways(pose, dx=0.5, yaw=0.0):
    """The camera of `pose` (None: the identity) moved dx metres along its own x axis and turned by yaw about its own y axis."""
    M = np.eye(4)
    M[0, 0], M[0, 2], M[2, 0], M[2, 2], M[0, 3] = math.cos(yaw), math.sin(yaw), -math.sin(yaw), math.cos(yaw), dx
    return (np.eye(4) if pose is None else np.asarray(pose, np.float64)) @ M
