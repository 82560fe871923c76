"""The frame-to-model alignment of include/viso_hip.h ("TSDF align") restated in numpy, twice: the linearise vectorised over the
pixels, and as a literal per-pixel loop in Python floats and ints; the loop of the alignment around it, in Python floats with the
header's operand order (the Cholesky factor, the two triangular solves, the increment), so that a device trace can be followed step
by step; and an unquantised variant of the linearise (the rows in double, never rounded) for the comparison of what the integers cost.

The map is an entry array (tests/tsdf_ref.py's ENTRY) sorted by key.  voxel and s = voxel / 1024 in double, G = gate_voxels 1024.0.
Everything is IEEE double in the operand order written, no fused multiply-add.
  1. A pixel contributes by rules 1 and 2 of the TSDF map with the map's min_disp16: P = (X, Y, Z).  n_points += 1.
  2. Q_i = ((T[i][0] X + T[i][1] Y) + T[i][2] Z) + T[i][3]; no pose: the identity matrix.
  3. u_i = Q_i / voxel - 0.5, k0_i = floor(u_i), t_i = u_i - k0_i.  u_i not finite or k0_i outside -2^20 .. 2^20 - 2:
     n_out_of_range += 1, skipped.
  4. The eight voxels k0 + (dx, dy, dz); usable: in the table with weight >= min_weight.  Any not usable: n_missing += 1, skipped.
     m[dz][dy][dx] = float64(sum) / float64(weight).
  5. X1[dz][dy] = m[dz][dy][1] - m[dz][dy][0], X0[dz][dy] = m[dz][dy][0] + t_0 X1[dz][dy];
     Y1[dz] = X0[dz][1] - X0[dz][0], Y0[dz] = X0[dz][0] + t_1 Y1[dz], YX[dz] = X1[dz][0] + t_1 (X1[dz][1] - X1[dz][0]);
     psi = Y0[0] + t_2 (Y0[1] - Y0[0]), D0 = YX[0] + t_2 (YX[1] - YX[0]), D1 = Y1[0] + t_2 (Y1[1] - Y1[0]), D2 = Y0[1] - Y0[0];
     g_i = D_i / 1024.
  6. |psi| > G: n_gated += 1, skipped.
  7. w = (f base) / (Z Z), e = (psi s) w, c_j = (T[0][j] g_0 + T[1][j] g_1) + T[2][j] g_2,
     a = (c_0 w, c_1 w, c_2 w, (Y c_2 - Z c_1) w, (Z c_0 - X c_2) w, (X c_1 - Y c_0) w).
  8. A_i = floor(a_i 256 + 0.5), A_6 = floor(e 256 + 0.5); not finite or |A_i| >= 2^20: n_clipped += 1, skipped.
  9. n_used += 1, N[i][j] += A_i A_j.
The alignment: steps a..f of the header (align, step)."""
import math

import numpy as np

from map_ref import BIAS, INVALID, keys_of, scale

COUNTERS = ("n_points", "n_used", "n_missing", "n_gated", "n_clipped", "n_out_of_range")
DEFAULTS = dict(min_weight=2, gate_voxels=1.0, max_iters=10, eps_rot=1e-6, eps_trans=1e-5, min_pixels=200)
K_LO, K_HI = -BIAS, BIAS - 2
CLIP = float(1 << 20)
RULES = ("invalid", "out_of_range", "missing", "gated", "clipped", "used")   # what ended a pixel, for the loop's trace


def _pose(pose):
    T = np.eye(4) if pose is None else np.array(pose, np.float64)
    assert T.shape == (4, 4) and np.isfinite(T[:3]).all()
    return T


def trilinear(m, t):
    """Step 5 on m[dz][dy][dx] (any array shape behind the three corner axes) and t = (t_0, t_1, t_2): (psi, (D0, D1, D2))."""
    X1 = [[m[dz][dy][1] - m[dz][dy][0] for dy in range(2)] for dz in range(2)]
    X0 = [[m[dz][dy][0] + t[0] * X1[dz][dy] for dy in range(2)] for dz in range(2)]
    Y1 = [X0[dz][1] - X0[dz][0] for dz in range(2)]
    Y0 = [X0[dz][0] + t[1] * Y1[dz] for dz in range(2)]
    YX = [X1[dz][0] + t[1] * (X1[dz][1] - X1[dz][0]) for dz in range(2)]
    D2 = Y0[1] - Y0[0]
    psi = Y0[0] + t[2] * D2
    D0 = YX[0] + t[2] * (YX[1] - YX[0])
    D1 = Y1[0] + t[2] * (Y1[1] - Y1[0])
    return psi, (D0, D1, D2)


def _matrix(n28):
    N = np.zeros((7, 7), n28.dtype)
    iu = np.triu_indices(7)
    N[iu] = n28
    N.T[iu] = n28
    return N


def linearize(entries, voxel, m, param, pose=None, min_weight=2, gate_voxels=1.0, min_disp16=16, quantize=True):
    """(N [7][7] symmetric, counters dict), vectorised.  quantize: N is int64, the contract.  Without it the rows are never rounded
    and nothing is clipped: N is float64, the sums of a_i a_j 65536 (so that N / 65536 is H, b, C either way)."""
    m = np.asarray(m)
    assert m.dtype == np.int16 and m.ndim == 2 and min_disp16 >= 1 and min_weight >= 1
    keys = keys_of(entries["k"])
    assert (np.diff(keys) > 0).all()
    T = _pose(pose)
    s, vox, gate = scale(voxel), np.float64(voxel), np.float64(gate_voxels) * np.float64(1024.0)
    f, cu, cv, base = (np.float64(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    use = (m != INVALID) & (m >= min_disp16)
    y, x = (a.astype(np.float64) for a in np.nonzero(use))
    c = dict.fromkeys(COUNTERS, 0)
    c["n_points"] = int(use.sum())
    with np.errstate(all="ignore"):
        d = m[use].astype(np.float64) / 16.0
        P = [(base * (x - cu)) / d, (base * (y - cv)) / d, (f * base) / d]
        u = [(((T[i, 0] * P[0]) + (T[i, 1] * P[1])) + (T[i, 2] * P[2])) + T[i, 3] for i in range(3)]
        u = np.stack([q / vox - 0.5 for q in u], axis=-1)
        k0 = np.floor(u)
        inr = ((k0 >= K_LO) & (k0 <= K_HI)).all(axis=1)            # False for a NaN and an infinity
        c["n_out_of_range"] = int((~inr).sum())
        P, u, k0 = [p[inr] for p in P], u[inr], k0[inr]
        t = [u[:, i] - k0[:, i] for i in range(3)]
        k0 = k0.astype(np.int64)
        usable = np.ones(len(k0), bool)
        mm = [[[None, None], [None, None]], [[None, None], [None, None]]]
        for dz in range(2):
            for dy in range(2):
                for dx in range(2):
                    want = keys_of(k0 + np.array([dx, dy, dz]))
                    at = np.minimum(np.searchsorted(keys, want), max(len(keys) - 1, 0))
                    hit = (keys[at] == want) & (entries["weight"][at] >= min_weight) if len(keys) else np.zeros(len(k0), bool)
                    usable &= hit
                    mm[dz][dy][dx] = (entries["sum"][at].astype(np.float64) / entries["weight"][at].astype(np.float64) if len(keys)
                                      else np.zeros(len(k0)))
        c["n_missing"] = int((~usable).sum())
        psi, D = trilinear(mm, t)
        gated = usable & (np.abs(psi) > gate)
        c["n_gated"] = int(gated.sum())
        ok = usable & ~gated
        g = [Di / 1024.0 for Di in D]
        X, Y, Z = P
        w = (f * base) / (Z * Z)
        e = (psi * s) * w
        cc = [((T[0, j] * g[0]) + (T[1, j] * g[1])) + (T[2, j] * g[2]) for j in range(3)]
        a = [cc[0] * w, cc[1] * w, cc[2] * w, (Y * cc[2] - Z * cc[1]) * w, (Z * cc[0] - X * cc[2]) * w, (X * cc[1] - Y * cc[0]) * w, e]
        if not quantize:
            A = np.stack(a, axis=-1)[ok] * 256.0
            c["n_used"] = int(ok.sum())
            return A.T @ A, c
        A = np.stack([np.floor(v * 256.0 + 0.5) for v in a], axis=-1)
        clipped = ok & ~(np.abs(A) < CLIP).all(axis=1)              # a NaN is clipped
        c["n_clipped"] = int(clipped.sum())
        ok &= ~clipped
        c["n_used"] = int(ok.sum())
        A = A[ok].astype(np.int64)
    iu = np.triu_indices(7)
    return _matrix((A[:, iu[0]] * A[:, iu[1]]).sum(axis=0, dtype=np.int64)), c


def linearize_loop(entries, voxel, m, param, pose=None, min_weight=2, gate_voxels=1.0, min_disp16=16, trace=None):
    """The same, one pixel at a time, in Python floats and ints.  trace: a Counter of RULES, which rule ended each pixel."""
    m = np.asarray(m)
    table = {int(k): (int(w), int(q)) for k, w, q in zip(keys_of(entries["k"]), entries["weight"], entries["sum"])}
    T = [[float(v) for v in row] for row in _pose(pose)]
    s, vox, gate = float(voxel) / 1024.0, float(voxel), float(gate_voxels) * 1024.0
    f, cu, cv, base = (float(getattr(param, k)) for k in ("f", "cu", "cv", "base"))
    N = [[0] * 7 for _ in range(7)]
    c = dict.fromkeys(COUNTERS, 0)

    def end(rule, counter=None):
        if trace is not None:
            trace[rule] += 1
        if counter:
            c[counter] += 1

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
            for dz in range(2):
                for dy in range(2):
                    for dx in range(2):
                        rec = table.get(((k0[0] + dx + BIAS) << 42) | ((k0[1] + dy + BIAS) << 21) | (k0[2] + dz + BIAS))
                        if rec is not None and rec[0] >= min_weight:
                            mm[dz][dy][dx] = float(rec[1]) / float(rec[0])
            if any(v is None for plane in mm for row in plane for v in row):
                end("missing", "n_missing")
                continue
            psi, D = trilinear(mm, t)
            if abs(psi) > gate:
                end("gated", "n_gated")
                continue
            g = [Di / 1024.0 for Di in D]
            w = (f * base) / (Z * Z)
            e = (psi * s) * w
            cc = [(T[0][j] * g[0] + T[1][j] * g[1]) + T[2][j] * g[2] for j in range(3)]
            a = [cc[0] * w, cc[1] * w, cc[2] * w, (Y * cc[2] - Z * cc[1]) * w, (Z * cc[0] - X * cc[2]) * w, (X * cc[1] - Y * cc[0]) * w, e]
            r = [v * 256.0 + 0.5 for v in a]
            if not all(math.isfinite(v) for v in r) or any(abs(math.floor(v)) >= 1 << 20 for v in r):
                end("clipped", "n_clipped")
                continue
            A = [math.floor(v) for v in r]
            end("used", "n_used")
            for i in range(7):
                for j in range(7):
                    N[i][j] += A[i] * A[j]
    assert all(abs(v) < 1 << 63 for row in N for v in row)
    return np.array(N, np.int64), c


# ---- the alignment: steps a..f in Python floats ---------------------------------------------------------------------------------
def cholesky(H):
    """Step c: the lower factor as a list of rows, or None when a pivot is not greater than 1e-12 times its diagonal entry."""
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        d = H[j][j]
        for k in range(j):
            d -= L[j][k] * L[j][k]
        if not d > 1e-12 * H[j][j]:
            return None
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            v = H[i][j]
            for k in range(j):
                v -= L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    return L


def solve(L, r):
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        v = r[i]
        for k in range(i):
            v -= L[i][k] * y[k]
        y[i] = v / L[i][i]
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v -= L[k][i] * x[k]
        x[i] = v / L[i][i]
    return x


def increment(T, xi):
    """Step e: T D(xi) as a 4 x 4 array, xi = (v, omega)."""
    T = [[float(v) for v in row] for row in np.asarray(T, np.float64)]
    v, w = [float(q) for q in xi[:3]], [float(q) for q in xi[3:]]
    theta2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    theta = math.sqrt(theta2)
    if theta < 1e-8:
        A, B = 1.0 - theta2 / 6.0, 0.5 - theta2 / 24.0
    else:
        A, B = math.sin(theta) / theta, (1.0 - math.cos(theta)) / theta2
    K = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    D = [[((1.0 if i == j else 0.0) + A * K[i][j]) + B * (w[i] * w[j] - (theta2 if i == j else 0.0)) for j in range(3)] + [v[i]]
         for i in range(3)]
    out = np.eye(4)
    for i in range(3):
        for j in range(4):
            r = (T[i][0] * D[0][j] + T[i][1] * D[1][j]) + T[i][2] * D[2][j]
            out[i, j] = r + T[i][3] if j == 3 else r
    return out


def system(N, n_used, min_pixels):
    """Steps a..c on a linearise: (status 0 / -1 / -2, H rows, b, C, L)."""
    N = np.asarray(N)
    H = [[float(N[i][j]) / 65536.0 for j in range(6)] for i in range(6)]
    b = [float(N[i][6]) / 65536.0 for i in range(6)]
    C = float(N[6][6]) / 65536.0
    if n_used < min_pixels:
        return -1, H, b, C, None
    L = cholesky(H)
    return (0 if L is not None else -2), H, b, C, L


def step(N, n_used, T, min_pixels=200):
    """Steps a..e from one linearise: (status, xi, the next pose); status 0: a step was taken, else -1, -2 or -3 and T is unchanged."""
    st, _, b, _, L = system(N, n_used, min_pixels)
    if st:
        return st, None, np.array(T, np.float64)
    xi = [-v for v in solve(L, b)]
    if not all(math.isfinite(v) for v in xi):
        return -3, xi, np.array(T, np.float64)
    return 0, xi, increment(T, xi)


def align(entries, voxel, m, param, pose=None, min_disp16=16, quantize=True, linearize_fn=None, **params):
    """The loop of viso_tsdf_align.  Returns (record dict: pose, cov, cost, n_used, iters, status; steps: [(pose, N, counters)] of
    every linearise, the last one included)."""
    p = dict(DEFAULTS, **params)
    guess = _pose(pose)
    T = guess.copy()
    T[3] = 0, 0, 0, 1
    steps = []

    def lin(T):
        if linearize_fn is not None:
            N, c = linearize_fn(T)
        else:
            N, c = linearize(entries, voxel, m, param, T, p["min_weight"], p["gate_voxels"], min_disp16, quantize)
        steps.append((T.copy(), N, c))
        return N, c

    def failed(status):
        return dict(pose=guess, cov=np.zeros((6, 6)), cost=0.0, n_used=0, iters=0, status=status), steps

    iters, status = 0, 2
    for _ in range(p["max_iters"]):
        N, c = lin(T)
        st, xi, T = step(N, c["n_used"], T, p["min_pixels"])
        if st:
            return failed(st)
        iters += 1
        nv = math.sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2])
        nw = math.sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5])
        if nw <= p["eps_rot"] and nv <= p["eps_trans"]:
            status = 1
            break
    N, c = lin(T)
    st, _, _, C, L = system(N, c["n_used"], p["min_pixels"])
    if st:
        return failed(st)
    n_used = c["n_used"]
    sigma2 = C / (float(n_used - 6) if n_used > 7 else 1.0)
    cov = np.zeros((6, 6))
    for j in range(6):
        col = solve(L, [1.0 if i == j else 0.0 for i in range(6)])
        for i in range(6):
            cov[i, j] = sigma2 * col[i]
    return dict(pose=T, cov=cov, cost=math.sqrt(C / float(n_used)), n_used=n_used, iters=iters, status=status), steps


def pose_error(T, truth):
    """(rotation in degrees, translation in metres) of T against truth."""
    T, truth = np.asarray(T, np.float64), np.asarray(truth, np.float64)
    R = truth[:3, :3].T @ T[:3, :3]
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(R) - 1.0) / 2.0))))
    return ang, float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))
