"""The photometric frame-to-model alignment of include/viso_hip.h ("TSDF photometric align") restated in numpy, twice: the linearise
vectorised over the pixels, and as a literal per-pixel loop in Python floats and ints.  Both restate the geometric steps 1..9 of
"TSDF align" themselves (tests/align_ref.py's linearize is not used here, so that "the geometric row is the plain one" is a check
of two texts); the loop of the alignment around them is align_ref.align's, given the linearise.

The map is a gray entry array (tests/gray_ref.py's ENTRY) sorted by key, the image uint8 of the map's shape.  Everything is IEEE
double in the operand order written, no fused multiply-add.  A pixel is *used* by steps 1..8 of "TSDF align"; its geometric row A
adds A_i A_j to N.  Then, for a used pixel, with lambda = photo_weight:
  P1. i[dz][dy][dx] = float64(gray) / float64(weight) of the same eight voxels.
  P2. step 5 on i with the same t: mu for psi, E_0..2 for D_0..2; h_i = E_i / voxel (gray levels per metre).
  P3. r = mu - float64(image[y][x]); |r| > photo_gate: n_photo_gated += 1, no photometric row.
  P4. hc_j = (T[0][j] h_0 + T[1][j] h_1) + T[2][j] h_2; b_0..2 = hc_j lambda, b_3..5 = (P x hc) lambda in step 7's order,
      b_6 = r lambda.
  P5. B_i = floor(b_i 256 + 0.5); not finite or |B_i| >= 2^20: n_photo_clipped += 1, no photometric row.
  P6. n_photo_used += 1, N[i][j] += B_i B_j, p += B_6 B_6."""
import math

import numpy as np

import align_ref as AR
from map_ref import BIAS, INVALID, keys_of, scale

PHOTO_COUNTERS = ("n_photo_used", "n_photo_gated", "n_photo_clipped")
COUNTERS = AR.COUNTERS + PHOTO_COUNTERS
PHOTO_DEFAULTS = dict(photo_weight=1.0 / 32.0, photo_gate=255.0)
RULES = AR.RULES + ("photo_gated", "photo_clipped", "photo_used")   # a used pixel also ends in one of the last three
K_LO, K_HI = -BIAS, BIAS - 2
CLIP = float(1 << 20)


def _pose(pose):
    T = np.eye(4) if pose is None else np.array(pose, np.float64)
    assert T.shape == (4, 4) and np.isfinite(T[:3]).all()
    return T


def interpolate(m, t):
    """Step 5 on m[dz][dy][dx] and t = (t_0, t_1, t_2): (the value, (its derivative per voxel along x, y, z))."""
    X1 = [[m[dz][dy][1] - m[dz][dy][0] for dy in range(2)] for dz in range(2)]
    X0 = [[m[dz][dy][0] + t[0] * X1[dz][dy] for dy in range(2)] for dz in range(2)]
    Y1 = [X0[dz][1] - X0[dz][0] for dz in range(2)]
    Y0 = [X0[dz][0] + t[1] * Y1[dz] for dz in range(2)]
    YX = [X1[dz][0] + t[1] * (X1[dz][1] - X1[dz][0]) for dz in range(2)]
    D2 = Y0[1] - Y0[0]
    return Y0[0] + t[2] * D2, (YX[0] + t[2] * (YX[1] - YX[0]), Y1[0] + t[2] * (Y1[1] - Y1[0]), D2)


def _matrix(n28):
    N = np.zeros((7, 7), np.int64)
    iu = np.triu_indices(7)
    N[iu] = n28
    N.T[iu] = n28
    return N


def _products(A):
    iu = np.triu_indices(7)
    return (A[:, iu[0]] * A[:, iu[1]]).sum(axis=0, dtype=np.int64)


def linearize(entries, voxel, m, image, param, pose=None, min_weight=2, gate_voxels=1.0, photo_weight=1.0 / 32.0, photo_gate=255.0,
              min_disp16=16):
    """(N [7][7] symmetric int64, p, counters dict of COUNTERS), vectorised."""
    m, image = np.asarray(m), np.asarray(image)
    assert m.dtype == np.int16 and m.ndim == 2 and image.dtype == np.uint8 and image.shape == m.shape
    assert min_disp16 >= 1 and min_weight >= 1 and math.isfinite(photo_weight) and photo_weight >= 0 and photo_gate > 0
    keys = keys_of(entries["k"])
    assert (np.diff(keys) > 0).all()
    T = _pose(pose)
    s, vox, gate = scale(voxel), np.float64(voxel), np.float64(gate_voxels) * np.float64(1024.0)
    lam, pgate = np.float64(photo_weight), np.float64(photo_gate)
    f, cu, cv, base = (np.float64(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    use = (m != INVALID) & (m >= min_disp16)
    y, x = (a.astype(np.float64) for a in np.nonzero(use))
    pix = image[use].astype(np.float64)
    c = dict.fromkeys(COUNTERS, 0)
    c["n_points"] = int(use.sum())
    with np.errstate(all="ignore"):
        d = m[use].astype(np.float64) / 16.0
        P = [(base * (x - cu)) / d, (base * (y - cv)) / d, (f * base) / d]
        u = [(((T[i, 0] * P[0]) + (T[i, 1] * P[1])) + (T[i, 2] * P[2])) + T[i, 3] for i in range(3)]
        u = np.stack([q / vox - 0.5 for q in u], axis=-1)
        k0 = np.floor(u)
        inr = ((k0 >= K_LO) & (k0 <= K_HI)).all(axis=1)
        c["n_out_of_range"] = int((~inr).sum())
        P, u, k0, pix = [q[inr] for q in P], u[inr], k0[inr], pix[inr]
        t = [u[:, i] - k0[:, i] for i in range(3)]
        k0 = k0.astype(np.int64)
        usable = np.ones(len(k0), bool)
        mm = [[[None, None], [None, None]], [[None, None], [None, None]]]
        ii = [[[None, None], [None, None]], [[None, None], [None, None]]]
        for dz in range(2):
            for dy in range(2):
                for dx in range(2):
                    if not len(keys):
                        usable[:] = False
                        mm[dz][dy][dx] = ii[dz][dy][dx] = np.zeros(len(k0))
                        continue
                    want = keys_of(k0 + np.array([dx, dy, dz]))
                    at = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
                    usable &= (keys[at] == want) & (entries["weight"][at] >= min_weight)
                    wgt = entries["weight"][at].astype(np.float64)
                    mm[dz][dy][dx] = entries["sum"][at].astype(np.float64) / wgt
                    ii[dz][dy][dx] = entries["gray"][at].astype(np.float64) / wgt
        c["n_missing"] = int((~usable).sum())
        psi, D = interpolate(mm, t)
        gated = usable & (np.abs(psi) > gate)
        c["n_gated"] = int(gated.sum())
        ok = usable & ~gated
        g = [Di / 1024.0 for Di in D]
        X, Y, Z = P
        w = (f * base) / (Z * Z)
        e = (psi * s) * w
        cc = [((T[0, j] * g[0]) + (T[1, j] * g[1])) + (T[2, j] * g[2]) for j in range(3)]
        a = [cc[0] * w, cc[1] * w, cc[2] * w, (Y * cc[2] - Z * cc[1]) * w, (Z * cc[0] - X * cc[2]) * w, (X * cc[1] - Y * cc[0]) * w, e]
        A = np.stack([np.floor(v * 256.0 + 0.5) for v in a], axis=-1)
        clipped = ok & ~(np.abs(A) < CLIP).all(axis=1)
        c["n_clipped"] = int(clipped.sum())
        ok &= ~clipped
        c["n_used"] = int(ok.sum())
        n28 = _products(A[ok].astype(np.int64))
        # the photometric row of the used pixels
        mu, E = interpolate(ii, t)
        h = [Ei / vox for Ei in E]
        r = mu - pix
        pg = ok & (np.abs(r) > pgate)
        c["n_photo_gated"] = int(pg.sum())
        hc = [((T[0, j] * h[0]) + (T[1, j] * h[1])) + (T[2, j] * h[2]) for j in range(3)]
        b = [hc[0] * lam, hc[1] * lam, hc[2] * lam, (Y * hc[2] - Z * hc[1]) * lam, (Z * hc[0] - X * hc[2]) * lam,
             (X * hc[1] - Y * hc[0]) * lam, r * lam]
        B = np.stack([np.floor(v * 256.0 + 0.5) for v in b], axis=-1)
        pok = ok & ~pg
        pc = pok & ~(np.abs(B) < CLIP).all(axis=1)
        c["n_photo_clipped"] = int(pc.sum())
        pok &= ~pc
        c["n_photo_used"] = int(pok.sum())
        B = B[pok].astype(np.int64)
    return _matrix(n28 + _products(B)), int((B[:, 6] * B[:, 6]).sum(dtype=np.int64)), c


def linearize_loop(entries, voxel, m, image, param, pose=None, min_weight=2, gate_voxels=1.0, photo_weight=1.0 / 32.0, photo_gate=255.0,
                   min_disp16=16, trace=None):
    """The same, one pixel at a time, in Python floats and ints.  trace: a Counter of RULES: which rule ended each pixel, and for a
    used pixel also what became of its photometric row."""
    m, image = np.asarray(m), np.asarray(image)
    table = {int(k): (int(w), int(q), int(g)) for k, w, q, g in zip(keys_of(entries["k"]), entries["weight"], entries["sum"], entries["gray"])}
    T = [[float(v) for v in row] for row in _pose(pose)]
    s, vox, gate = float(voxel) / 1024.0, float(voxel), float(gate_voxels) * 1024.0
    lam, pgate = float(photo_weight), float(photo_gate)
    f, cu, cv, base = (float(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    N = [[0] * 7 for _ in range(7)]
    p = 0
    c = dict.fromkeys(COUNTERS, 0)

    def end(rule, counter=None):
        if trace is not None:
            trace[rule] += 1
        if counter:
            c[counter] += 1

    def rounded(row):
        r = [v * 256.0 + 0.5 for v in row]
        if not all(math.isfinite(v) for v in r) or any(abs(math.floor(v)) >= 1 << 20 for v in r):
            return None
        return [math.floor(v) for v in r]

    for y in range(m.shape[0]):
        for x in range(m.shape[1]):
            d16 = int(m[y, x])
            if d16 == INVALID or d16 < min_disp16:
                end("invalid")
                continue
            c["n_points"] += 1
            d = d16 / 16.0
            X, Y, Z = base * (x - cu) / d, base * (y - cv) / d, f * base / d
            u = [(((T[i][0] * X + T[i][1] * Y) + T[i][2] * Z) + T[i][3]) / vox - 0.5 for i in range(3)]
            if not all(math.isfinite(v) for v in u) or any(not K_LO <= math.floor(v) <= K_HI for v in u):
                end("out_of_range", "n_out_of_range")
                continue
            k0 = [math.floor(v) for v in u]
            t = [v - k for v, k in zip(u, k0)]
            mm = [[[None, None], [None, None]], [[None, None], [None, None]]]
            ii = [[[None, None], [None, None]], [[None, None], [None, None]]]
            for dz in range(2):
                for dy in range(2):
                    for dx in range(2):
                        rec = table.get(((k0[0] + dx + BIAS) << 42) | ((k0[1] + dy + BIAS) << 21) | (k0[2] + dz + BIAS))
                        if rec is not None and rec[0] >= min_weight:
                            mm[dz][dy][dx] = float(rec[1]) / float(rec[0])
                            ii[dz][dy][dx] = float(rec[2]) / float(rec[0])
            if any(v is None for plane in mm for row in plane for v in row):
                end("missing", "n_missing")
                continue
            psi, D = interpolate(mm, t)
            if abs(psi) > gate:
                end("gated", "n_gated")
                continue
            g = [Di / 1024.0 for Di in D]
            w = (f * base) / (Z * Z)
            e = (psi * s) * w
            cc = [(T[0][j] * g[0] + T[1][j] * g[1]) + T[2][j] * g[2] for j in range(3)]
            A = rounded([cc[0] * w, cc[1] * w, cc[2] * w, (Y * cc[2] - Z * cc[1]) * w, (Z * cc[0] - X * cc[2]) * w,
                         (X * cc[1] - Y * cc[0]) * w, e])
            if A is None:
                end("clipped", "n_clipped")
                continue
            end("used", "n_used")
            for i in range(7):
                for j in range(7):
                    N[i][j] += A[i] * A[j]
            mu, E = interpolate(ii, t)
            h = [Ei / vox for Ei in E]
            r = mu - float(int(image[y, x]))
            if abs(r) > pgate:
                end("photo_gated", "n_photo_gated")
                continue
            hc = [(T[0][j] * h[0] + T[1][j] * h[1]) + T[2][j] * h[2] for j in range(3)]
            B = rounded([hc[0] * lam, hc[1] * lam, hc[2] * lam, (Y * hc[2] - Z * hc[1]) * lam, (Z * hc[0] - X * hc[2]) * lam,
                         (X * hc[1] - Y * hc[0]) * lam, r * lam])
            if B is None:
                end("photo_clipped", "n_photo_clipped")
                continue
            end("photo_used", "n_photo_used")
            for i in range(7):
                for j in range(7):
                    N[i][j] += B[i] * B[j]
            p += B[6] * B[6]
    assert all(abs(v) < 1 << 63 for row in N for v in row)
    return np.array(N, np.int64), p, c


def record(last, status, iters, photo_weight):
    """The record of viso_tsdf_align_gray from the last linearise (pose, N, counters with "p"): align_ref.align's with the
    covariance's divisor max(n_used + n_photo_used - 6, 1), and cost_geo (px), cost_photo (gray levels), n_photo_used."""
    T, N, c = last
    _, _, _, C, L = AR.system(N, c["n_used"], 0)
    n_used, n_photo = c["n_used"], c["n_photo_used"]
    tot = n_used + n_photo
    sigma2 = C / (float(tot - 6) if tot > 7 else 1.0)
    cov = np.zeros((6, 6))
    for j in range(6):
        col = AR.solve(L, [1.0 if i == j else 0.0 for i in range(6)])
        for i in range(6):
            cov[i, j] = sigma2 * col[i]
    pp = float(c["p"]) / 65536.0
    cost_photo = math.sqrt(pp / float(n_photo)) / float(photo_weight) if n_photo and photo_weight > 0 else 0.0
    return dict(pose=T, cov=cov, cost=math.sqrt(C / float(n_used)), n_used=n_used, iters=iters, status=status,
                cost_geo=math.sqrt((C - pp) / float(n_used)), cost_photo=cost_photo, n_photo_used=n_photo)


def align(entries, voxel, m, image, param, pose=None, min_disp16=16, photo_weight=1.0 / 32.0, photo_gate=255.0, loop=False, **params):
    """The loop of viso_tsdf_align_gray: align_ref.align around this file's linearise.  Returns (record dict, steps
    [(pose, N, counters with "p")])."""
    p = dict(AR.DEFAULTS, **params)
    fn = linearize_loop if loop else linearize

    def lin(T):
        N, pp, c = fn(entries, voxel, m, image, param, T, p["min_weight"], p["gate_voxels"], photo_weight, photo_gate, min_disp16)
        return N, dict(c, p=pp)

    rec, steps = AR.align(None, voxel, m, param, pose, min_disp16, linearize_fn=lin, **params)
    if rec["status"] < 0:
        return dict(rec, cost_geo=0.0, cost_photo=0.0, n_photo_used=0), steps
    return record(steps[-1], rec["status"], rec["iters"], photo_weight), steps
