"""numpy restatement of the opt-in motion covariance (include/viso_hip.h, "motion covariance"): the per-frame record,
the fully converged weighted least squares it describes, the triangulation, and the trajectory propagation of
viso_chain_covariances.  Vectorised over the points; the order of the sums is numpy's, not the kernel's."""
import numpy as np

from libviso_amd import hostmath

def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rot(tr):
    return hostmath.tr2mat(tr)[:3, :3]


def omega(tr):
    """W: columns w_i with dR/dr_i = [w_i]x R (R = Rx Ry Rz, tr2mat's order)."""
    sx, cx, sy, cy = np.sin(tr[0]), np.cos(tr[0]), np.sin(tr[1]), np.cos(tr[1])
    return np.array([[1.0, 0.0, sy], [0.0, cx, -sx * cy], [0.0, sx, cx * cy]])


def predict(X, tr, param):
    """pred (4, n) of the points X (3, n) under tr; also Xc (3, n)."""
    R = rot(tr)
    Xc = R @ X + np.asarray(tr[3:6])[:, None]
    f, cu, cv, b = param.f, param.cu, param.cv, param.base
    pred = np.stack([f * Xc[0] / Xc[2] + cu, f * Xc[1] / Xc[2] + cv, f * (Xc[0] - b) / Xc[2] + cu, f * Xc[1] / Xc[2] + cv])
    return pred, Xc


def triangulate(x, param):
    """triangulate_rectified (src/viso.cpp:1137-1162): x (4, n) = (uL, vL, uR, vR) -> X (3, n)."""
    f, cu, cv, b = param.f, param.cu, param.cv, param.base
    d = x[0] - x[2]
    return np.stack([(x[0] - cu) * b / d, (x[1] - cv) * b / d, f * b / d])


def terms(X, obs, tr, inl, param):
    """Per inlier j (k = inl[j]): J (n, 4, 6), r (n, 4), w (n,), M (n, 4, 3)."""
    tr = np.asarray(tr, np.float64)
    inl = np.asarray(inl, np.int64)
    n = len(inl)
    f, cu, b = param.f, param.cu, param.base
    R = rot(tr)
    Xp = X[:, inl]
    pred, Xc = predict(Xp, tr, param)
    r = (obs[:, inl] - pred).T
    w = 1.0 / (np.abs(obs[0, :n] - cu) / abs(cu) + 0.05)   # column j, not k (Q6)
    Zc = Xc[2]
    Pc = np.zeros((n, 4, 3))
    Pc[:, 0, 0] = f / Zc
    Pc[:, 0, 2] = -f * Xc[0] / Zc ** 2
    Pc[:, 1, 1] = f / Zc
    Pc[:, 1, 2] = -f * Xc[1] / Zc ** 2
    Pc[:, 2, 0] = f / Zc
    Pc[:, 2, 2] = -f * (Xc[0] - b) / Zc ** 2
    Pc[:, 3] = Pc[:, 1]
    W = omega(tr)
    dXc = np.zeros((n, 3, 6))
    for i in range(3):
        dXc[:, :, i] = (_skew(W[:, i]) @ R @ Xp).T
    dXc[:, :, 3:] = np.eye(3)
    J = Pc @ dXc
    d = f * b / Xp[2]
    T = np.zeros((n, 3, 3))
    T[:, 0, 0], T[:, 1, 0], T[:, 2, 0] = b / d - Xp[0] / d, -Xp[1] / d, -Xp[2] / d
    T[:, 1, 1] = b / d
    T[:, 0, 2], T[:, 1, 2], T[:, 2, 2] = Xp[0] / d, Xp[1] / d, Xp[2] / d
    M = Pc @ R @ T
    return J, r, w, M


def _chol_ok(A):
    """The kernel's test: every Cholesky pivot > 1e-12 x the original diagonal entry."""
    L = np.zeros((6, 6))
    for j in range(6):
        s = A[j, j] - L[j, :j] @ L[j, :j]
        if not s > 1e-12 * A[j, j]:
            return False
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return True


def motion_cov(X, obs, tr, inl, param, mode, sigma=None, ok=1, with_M=True):
    """The record of one frame as a dict (cov, delta, sigma2, gap, status, n)."""
    n = len(inl)
    rec = dict(cov=np.zeros((6, 6)), delta=np.zeros(6), sigma2=0.0, gap=0.0, status=0, n=n)
    if not ok:
        return rec
    if n < 6:
        rec["status"] = -1
        return rec
    J, r, w, M = terms(X, obs, tr, inl, param)
    if not with_M:
        M = np.zeros_like(M)
    w2, w4 = w ** 2, w ** 4
    JtJ = np.einsum("nri,nrj->nij", J, J)
    K = np.einsum("nrc,nrj->ncj", M, J)
    A = np.einsum("n,nij->ij", w2, JtJ)
    B = np.einsum("n,nij->ij", w4, JtJ + np.einsum("nci,ncj->nij", K, K))
    g = np.einsum("n,nri,nr->i", w2, J, r)
    if not (_chol_ok(A) and _chol_ok(B)):
        rec["status"] = -2
        return rec
    if mode == 2:
        s2 = float(sigma) ** 2
    else:
        s2 = float((r ** 2).sum() / (4.0 * n + (M ** 2).sum() - 6.0))
    Ai = np.linalg.inv(A)
    rec.update(cov=s2 * Ai @ B @ Ai, delta=Ai @ g, sigma2=s2, gap=float(g @ np.linalg.solve(B, g)) / s2 if s2 > 0 else 0.0,
               status=1)
    rec["cov"] = 0.5 * (rec["cov"] + rec["cov"].T)
    return rec


def wls(X, obs, inl, param, tr0, iters=50):
    """The fully converged weighted least squares with the estimator's weights (Gauss-Newton to machine precision)."""
    tr = np.array(tr0, np.float64)
    for _ in range(iters):
        J, r, w, _M = terms(X, obs, tr, inl, param)
        w2 = w ** 2
        A = np.einsum("n,nri,nrj->ij", w2, J, J)
        g = np.einsum("n,nri,nr->i", w2, J, r)
        step = np.linalg.solve(A, g)
        tr = tr + step
        if np.abs(step).max() < 1e-15:
            break
    return tr


def whitened_error(S_ref, S):
    """|S_ref^-1/2 S S_ref^-1/2 - I|_F."""
    ev, V = np.linalg.eigh(S_ref)
    Wh = V @ np.diag(ev ** -0.5) @ V.T
    return np.linalg.norm(Wh @ S @ Wh - np.eye(6))


# ---- trajectory propagation -----------------------------------------------------------------------------------------------
def adjoint(T):
    R, t = T[:3, :3], T[:3, 3]
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = R
    Ad[3:, 3:] = R
    Ad[3:, :3] = _skew(t) @ R
    return Ad


def G_analytic(tr):
    """d Log(T(tr^) inv(T(tr))) / d tr at tr^ = tr, xi = (phi, rho)."""
    W = omega(tr)
    G = np.zeros((6, 6))
    G[:3, :3] = -W
    G[3:, :3] = -_skew(np.asarray(tr[3:6])) @ W
    G[3:, 3:] = -np.eye(3)
    return G


def se3_log(T):
    """xi = (phi, rho) with T = Exp(xi)."""
    R, t = T[:3, :3], T[:3, 3]
    c = np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)
    th = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if th < 1e-6:
        phi = 0.5 * v
        a, bcoef = 0.5 - th ** 2 / 24.0, 1.0 / 6.0 - th ** 2 / 120.0
    else:
        phi = th / (2.0 * np.sin(th)) * v
        a, bcoef = (1.0 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    P = _skew(phi)
    V = np.eye(3) + a * P + bcoef * P @ P
    return np.concatenate([phi, np.linalg.solve(V, t)])


def G_numeric(tr, h=1e-6):
    tr = np.asarray(tr, np.float64)
    Th = hostmath.tr2mat(tr)
    G = np.zeros((6, 6))
    for i in range(6):
        e = np.zeros(6)
        e[i] = h
        G[:, i] = (se3_log(Th @ np.linalg.inv(hostmath.tr2mat(tr + e))) - se3_log(Th @ np.linalg.inv(hostmath.tr2mat(tr - e)))) / (2 * h)
    return G


def chain(tr, ok, covs):
    """(pose_cov [k][6][6], valid [k]) along hostmath.chain_poses' default list."""
    S = np.zeros((6, 6))
    out, valid = [S.copy()], [1]
    live = True
    for t in range(len(tr)):
        if not ok[t]:
            continue
        live = live and int(covs[t]["status"]) == 1
        if not live:
            out.append(np.zeros((6, 6)))
            valid.append(0)
            continue
        T = hostmath.tr2mat(tr[t])
        Ad, G = adjoint(T), G_analytic(tr[t])
        S = Ad @ S @ Ad.T + G @ np.asarray(covs[t]["cov"]).reshape(6, 6) @ G.T
        out.append(S.copy())
        valid.append(1)
    return np.array(out), np.array(valid, np.int32)
