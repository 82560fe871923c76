"""numpy restatement of the opt-in two-frame bundle adjustment (include/viso_hip.h, "motion refinement"): the
Schur-complement Levenberg-Marquardt over the motion and every used inlier's 3-D point, with the kernel's schedule, and the dense
(6 + 3n) Gauss-Newton system it reduces.  Vectorised over the points; the order of the sums is numpy's, not the kernel's."""
import numpy as np

import covariance_ref as CR

LAMBDA0, LAMBDA_MIN = 1e-4, 1e-12
MAX_ACCEPT, MAX_REJECT, REL_TOL = 20, 8, 1e-12


def used_points(X, inl):
    """L': the entries k of inl whose X[:, k] is finite with Z > 0, in inl's order."""
    inl = np.asarray(inl, np.int64)
    if len(inl) == 0:
        return inl
    P = X[:, inl]
    good = np.all(np.isfinite(P), axis=0) & (P[2] > 0)
    return inl[good]


def project0(P, param):
    """pi_0: the previous frame's (uL, vL, uR) of the points P (3, n) -- triangulate_rectified inverted."""
    f, cu, cv, b = param.f, param.cu, param.cv, param.base
    return np.stack([f * P[0] / P[2] + cu, f * P[1] / P[2] + cv, f * (P[0] - b) / P[2] + cu])


def blocks(P, tr, z0, z1, param):
    """Per point: J (n, 4, 6), Jx (n, 4, 3), P0 (n, 3, 3), r1 (n, 4), r0 (n, 3)."""
    n = P.shape[1]
    f, b = param.f, param.base
    R = CR.rot(tr)
    pred, Xc = CR.predict(P, tr, param)
    r1 = (z1 - pred).T
    r0 = (z0 - project0(P, param)).T
    Zc = Xc[2]
    Pc = np.zeros((n, 4, 3))
    Pc[:, 0, 0] = f / Zc
    Pc[:, 0, 2] = -f * Xc[0] / Zc ** 2
    Pc[:, 1, 1] = f / Zc
    Pc[:, 1, 2] = -f * Xc[1] / Zc ** 2
    Pc[:, 2, 0] = f / Zc
    Pc[:, 2, 2] = -f * (Xc[0] - b) / Zc ** 2
    Pc[:, 3] = Pc[:, 1]
    W = CR.omega(tr)
    dXc = np.zeros((n, 3, 6))
    for i in range(3):
        dXc[:, :, i] = (CR._skew(W[:, i]) @ R @ P).T
    dXc[:, :, 3:] = np.eye(3)
    J = Pc @ dXc
    Jx = Pc @ R
    Z = P[2]
    P0 = np.zeros((n, 3, 3))
    P0[:, 0, 0] = f / Z
    P0[:, 0, 2] = -f * P[0] / Z ** 2
    P0[:, 1, 1] = f / Z
    P0[:, 1, 2] = -f * P[1] / Z ** 2
    P0[:, 2, 0] = f / Z
    P0[:, 2, 2] = -f * (P[0] - b) / Z ** 2
    return J, Jx, P0, r1, r0


def cost(P, tr, z0, z1, param):
    pred, _ = CR.predict(P, tr, param)
    return float(((z1 - pred) ** 2).sum() + ((z0 - project0(P, param)) ** 2).sum())


def chol_ok(A):
    """The kernel's test: every Cholesky pivot > 1e-12 x the diagonal entry of the matrix factored."""
    k = A.shape[0]
    L = np.zeros_like(A)
    for j in range(k):
        s = A[j, j] - L[j, :j] @ L[j, :j]
        if not s > 1e-12 * A[j, j]:
            return False
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, k):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return True


def chol3_ok(A):
    """chol_ok of every 3 x 3 in A (n, 3, 3), vectorised."""
    with np.errstate(all="ignore"):
        a00, a11, a22 = A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]
        good = a00 > 1e-12 * a00
        l0 = np.sqrt(a00)
        l10, l20 = A[:, 1, 0] / l0, A[:, 2, 0] / l0
        p1 = a11 - l10 * l10
        good &= p1 > 1e-12 * a11
        l21 = (A[:, 2, 1] - l20 * l10) / np.sqrt(p1)
        p2 = a22 - l20 * l20 - l21 * l21
        good &= p2 > 1e-12 * a22
    return bool(np.all(good))


def normal_equations(P, tr, z0, z1, param, lam):
    """(S, s, Hpp_d (n, 3, 3), Hcp (n, 6, 3), gp (n, 3), ok): the reduced system with the diagonals of Hcc and of every Hpp_k
    multiplied by (1 + lam); ok is False when an Hpp_k or a point's I - M M' fails the Cholesky test."""
    J, Jx, P0, r1, r0 = blocks(P, tr, z0, z1, param)
    Hcc = np.einsum("nri,nrj->ij", J, J)
    Hcp = np.einsum("nri,nrc->nic", J, Jx)
    Hpp = np.einsum("nra,nrc->nac", Jx, Jx) + np.einsum("nra,nrc->nac", P0, P0)
    gc = np.einsum("nri,nr->i", J, r1)
    gp = np.einsum("nra,nr->na", Jx, r1) + np.einsum("nra,nr->na", P0, r0)
    Hcc_d = Hcc + lam * np.diag(np.diag(Hcc))
    Hpp_d = Hpp.copy()
    d = np.arange(3)
    Hpp_d[:, d, d] *= 1.0 + lam
    ok = chol3_ok(Hpp_d)
    if ok:
        # the kernel factors I - M M' (M = Jx~ l^-T, l = chol(Hpp_d), Jx~ = Jx's rows uL, sqrt(2) vL, uR): positive definite in
        # exact arithmetic, and held to the same pivot test
        Jxt = np.stack([Jx[:, 0], np.sqrt(2.0) * Jx[:, 1], Jx[:, 2]], axis=1)
        Lc = np.linalg.cholesky(Hpp_d)
        M = np.linalg.solve(Lc, np.transpose(Jxt, (0, 2, 1))).transpose(0, 2, 1)
        Q = np.eye(3) - M @ np.transpose(M, (0, 2, 1))
        ok = chol3_ok(Q)
    if not ok:
        return None, None, Hpp_d, Hcp, gp, False
    Hi = np.linalg.inv(Hpp_d)
    HcpHi = Hcp @ Hi
    S = Hcc_d - np.einsum("nic,njc->ij", HcpHi, Hcp)
    s = gc - np.einsum("nic,nc->i", HcpHi, gp)
    return 0.5 * (S + S.T), s, Hpp_d, Hcp, gp, True


ZERO_SLACK = dict(tr_abs=0.0, tr_white=0.0, pts_rel=0.0, pts_white=0.0)


def _empty(tr, status, n):
    return dict(tr=np.array(tr, np.float64), cov=np.zeros((6, 6)), sigma2=0.0, cost0=0.0, cost=0.0, gap=0.0, iters=0,
                status=status, n=n, points=np.zeros((3, 0)), idx=np.zeros(0, np.int64), trace=[], slack=dict(ZERO_SLACK))


def lm_step(P, tr, z0, z1, param, lam):
    """The step (dtr (6), dX (3, n)) of the damped system at (P, tr), or None where the loop would leave with -2 or -3."""
    S, s, Hpp_d, Hcp, gp, good = normal_equations(P, tr, z0, z1, param, lam)
    if not good or not (np.all(np.isfinite(S)) and np.all(np.isfinite(s))) or not chol_ok(S):
        return None
    dtr = np.linalg.solve(S, s)
    return dtr, np.linalg.solve(Hpp_d, (gp - np.einsum("nic,i->nc", Hcp, dtr))[:, :, None])[:, :, 0].T


def step_sizes(step, Cinv, Hpp, pmax):
    """A step's size per compared quantity: tr absolute (largest component) and whitened by cov = Cinv^-1, the points relative to
    pmax (the largest |coordinate| of the final points) and whitened, each by its own undamped Hpp (n, 3, 3); the largest point."""
    if step is None:
        return dict(ZERO_SLACK)
    dtr, dX = step
    return dict(tr_abs=float(np.abs(dtr).max()), tr_white=float(np.sqrt(dtr @ Cinv @ dtr)),
                pts_rel=float(np.abs(dX).max() / pmax),
                pts_white=float(np.sqrt(np.einsum("an,nac,cn->n", dX, Hpp, dX).max())))


def slack_of(last, further, Cinv, Hpp, pmax):
    """`slack`: per quantity, the larger of the last accepted step and of one further step from the final state -- how far a run
    whose last decisions fell the other way would end from this one."""
    a, b = step_sizes(last, Cinv, Hpp, pmax), step_sizes(further, Cinv, Hpp, pmax)
    return {k: max(a[k], b[k]) for k in a}


def refine(X, obs, tr, inl, param, mode, sigma=None, ok=1):
    """The record of one frame as a dict (tr, cov, sigma2, cost0, cost, gap, iters, status, n), plus the refined points (3, n),
    their indices idx (L'), `trace`: the relative cost change (C_new - C) / C of every accept / reject decision taken, and
    `slack` (slack_of): the size of the last accepted step and of one further step at the damping the loop would use next, and
    `Hpp` (n, 3, 3): every point's undamped block at the final state."""
    tr_in = np.array(tr, np.float64)
    Lp = used_points(X, inl)
    n = len(Lp)
    if not ok:
        return _empty(tr_in, 0, n)
    if n < 6:
        return _empty(tr_in, -1, n)
    P = X[:, Lp].astype(np.float64).copy()
    z1 = obs[:, Lp].astype(np.float64)
    cur_tr = tr_in.copy()
    with np.errstate(all="ignore"):
        z0 = project0(P, param)
        C = cost(P, cur_tr, z0, z1, param)
        cost0 = C
        lam, acc, rej = LAMBDA0, 0, 0
        trace, last = [], None
        if not np.isfinite(C):
            return _empty(tr_in, -3, n)
        while C != 0.0:
            S, s, Hpp_d, Hcp, gp, good = normal_equations(P, cur_tr, z0, z1, param, lam)
            if good and not (np.all(np.isfinite(S)) and np.all(np.isfinite(s))):
                return _empty(tr_in, -3, n)
            if not good or not chol_ok(S):
                return _empty(tr_in, -2, n)
            dtr = np.linalg.solve(S, s)
            dX = np.linalg.solve(Hpp_d, (gp - np.einsum("nic,i->nc", Hcp, dtr))[:, :, None])[:, :, 0].T
            tr_new, P_new = cur_tr + dtr, P + dX
            C_new = cost(P_new, tr_new, z0, z1, param)
            trace.append((C_new - C) / C)
            if C_new < C:
                acc += 1
                rej = 0
                lam = max(lam / 10.0, LAMBDA_MIN)
                stop = C - C_new <= REL_TOL * C or C_new == 0.0 or acc == MAX_ACCEPT
                cur_tr, P, C = tr_new, P_new, C_new
                last = (dtr, dX)
                if stop:
                    break
            else:
                lam *= 10.0
                rej += 1
                if rej == MAX_REJECT:
                    break
        S, s, Hpp, _c, _g, good = normal_equations(P, cur_tr, z0, z1, param, 0.0)
        if good and not (np.all(np.isfinite(S)) and np.all(np.isfinite(s))):
            return _empty(tr_in, -3, n)
        if not good or not chol_ok(S):
            return _empty(tr_in, -2, n)
        s2 = float(sigma) ** 2 if mode == 2 else C / (4.0 * n - 6.0)
        Si = np.linalg.inv(S)
        cov = s2 * 0.5 * (Si + Si.T)
        gap = float(s @ Si @ s) / s2 if s2 > 0 else 0.0
        if not (np.all(np.isfinite(cov)) and np.isfinite(gap) and np.all(np.isfinite(cur_tr)) and np.all(np.isfinite(P))):
            return _empty(tr_in, -3, n)
        further = lm_step(P, cur_tr, z0, z1, param, lam) if C != 0.0 else None
        slack = slack_of(last, further, S / max(s2, 1e-300), Hpp, float(np.abs(P).max()))
    return dict(tr=cur_tr, cov=cov, sigma2=s2, cost0=cost0, cost=C, gap=gap, iters=acc, status=1, n=n, points=P, idx=Lp,
                trace=trace, slack=slack, Hpp=Hpp)


def dense_hessian(P, tr, z0, z1, param):
    """The undamped Gauss-Newton Hessian (6 + 3n) of the full cost, tr first, then X_k in order, and its gradient J'r."""
    J, Jx, P0, r1, r0 = blocks(P, tr, z0, z1, param)
    n = P.shape[1]
    rows = 7 * n
    Jd = np.zeros((rows, 6 + 3 * n))
    r = np.zeros(rows)
    for k in range(n):
        Jd[4 * k:4 * k + 4, :6] = J[k]
        Jd[4 * k:4 * k + 4, 6 + 3 * k:9 + 3 * k] = Jx[k]
        r[4 * k:4 * k + 4] = r1[k]
        Jd[4 * n + 3 * k:4 * n + 3 * k + 3, 6 + 3 * k:9 + 3 * k] = P0[k]
        r[4 * n + 3 * k:4 * n + 3 * k + 3] = r0[k]
    return Jd.T @ Jd, Jd.T @ r
