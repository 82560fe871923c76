"""numpy restatement of the opt-in sliding-window bundle adjustment (include/viso_hip.h, "window refinement"): the
break rule and the anchor, the links and tracks, the Schur-complement Levenberg-Marquardt over the window's motions and every
track's point with the kernel's schedule, the record, and the dense Gauss-Newton system it reduces.  Vectorised over the tracks
of one (s, e) pattern; the order of the sums is numpy's, not the kernel's."""
import numpy as np

import covariance_ref as CR
import refine_ref as RR

LAMBDA0, LAMBDA_MIN = RR.LAMBDA0, RR.LAMBDA_MIN
MAX_ACCEPT, MAX_REJECT, REL_TOL = RR.MAX_ACCEPT, RR.MAX_REJECT, RR.REL_TOL
RT2 = np.sqrt(2.0)


class Frame:
    """One solved frame j >= 1: X = Xp_c (3, m), obs = x_c (4, m), left (m, 2) = (cur-left, prev-left) of every row, tr (6), ok,
    inl (the final inlier list)."""

    def __init__(self, X, obs, left, tr, ok, inl):
        self.X = np.asarray(X, np.float64)
        self.obs = np.asarray(obs, np.float64)
        self.left = np.asarray(left, np.int64).reshape(-1, 2)
        self.tr = np.asarray(tr, np.float64)
        self.ok = int(ok)
        self.inl = np.asarray(inl, np.int64)
        self.Lp = RR.used_points(self.X, self.inl)


def is_break(fr):
    return fr.ok == 0 or len(fr.Lp) < 6


def anchor(frames, t, K):
    """a = max(t - K + 1, 0, the largest break j < t); frames[0] is frame 0 (never read)."""
    a = max(t - K + 1, 0)
    for j in range(max(a, 1), t):
        if is_break(frames[j]):
            a = j
    return a


def _unique(keys, rows):
    """{key: row} for the keys held by exactly one row, {key: -2} for the others."""
    tab = {}
    for k, r in zip(keys, rows):
        tab[int(k)] = -2 if int(k) in tab else int(r)
    return tab


def tables(fr):
    """(by cur-left, by prev-left) over L'."""
    rows = fr.Lp
    return _unique(fr.left[rows, 0], rows), _unique(fr.left[rows, 1], rows)


def back_link(frames, tabs, j, r):
    """The row of L'_{j-1} that row r of L'_j links to, or -1."""
    p = int(frames[j].left[r, 1])
    if tabs[j][1].get(p, -1) != r:
        return -1
    q = tabs[j - 1][0].get(p, -1)
    return q if q >= 0 else -1


def fwd_link(frames, tabs, j, r):
    """The row of L'_{j+1} that links to row r of L'_j, or -1."""
    p = int(frames[j].left[r, 0])
    if tabs[j][0].get(p, -1) != r:
        return -1
    q = tabs[j + 1][1].get(p, -1)
    return q if q >= 0 else -1


def tracks(frames, a, t):
    """The window's tracks in the kernel's order: s ascending, then L'_{s+1}'s order.  Each is (s, [r_{s+1}, ..., r_e])."""
    tabs = {j: tables(frames[j]) for j in range(a + 1, t + 1)}
    out = []
    for s in range(a, t):
        j = s + 1
        for r in frames[j].Lp:
            r = int(r)
            if j > a + 1 and back_link(frames, tabs, j, r) >= 0:
                continue
            rows = [r]
            jj = j
            while jj < t:
                q = fwd_link(frames, tabs, jj, rows[-1])
                if q < 0:
                    break
                rows.append(q)
                jj += 1
            out.append((s, rows))
    return out


def _chain(trs):
    """A[j][i] = R_j ... R_{i+1} (A[j][j] = I), frames offset from the anchor."""
    n = len(trs) + 1
    Rs = [None] + [CR.rot(tr) for tr in trs]
    A = [[None] * n for _ in range(n)]
    for j in range(n):
        A[j][j] = np.eye(3)
        for i in range(j - 1, -1, -1):
            A[j][i] = A[j][i + 1] @ Rs[i + 1]
    return Rs, A


class Window:
    """The fixed data of one window: tracks grouped by (s, e) offsets from the anchor, their observations and starting points."""

    def __init__(self, frames, a, t, param):
        self.a, self.t, self.len, self.param = a, t, t - a + 1, param
        self.nc = 6 * (self.len - 1)
        trk = tracks(frames, a, t)
        self.order = trk
        self.n_points = len(trk)
        self.n_rows = sum(3 + 4 * len(rows) for _, rows in trk)
        groups = {}
        for k, (s, rows) in enumerate(trk):
            groups.setdefault((s - a, s - a + len(rows)), []).append(k)
        self.groups = []
        trs = [frames[j].tr for j in range(a + 1, t + 1)]
        for (so, eo), ks in sorted(groups.items()):
            z0, zs, P = [], [], []
            for k in ks:
                s, rows = trk[k]
                Xs = frames[s + 1].X[:, rows[0]]
                z0.append(RR.project0(Xs[:, None], param)[:, 0])
                zs.append(np.stack([frames[s + 1 + i].obs[:, r] for i, r in enumerate(rows)]))   # (e - s, 4)
                Y = Xs.copy()
                for i in range(so, 0, -1):                # T_s^-1: frame s -> frame a
                    Y = CR.rot(trs[i - 1]).T @ (Y - trs[i - 1][3:])
                P.append(Y)
            self.groups.append(dict(so=so, eo=eo, ks=np.array(ks), z0=np.array(z0).T, z=np.array(zs), P0=np.array(P).T))
        self.tr0 = np.array(trs)

    def start_points(self):
        return [g["P0"].copy() for g in self.groups]


def _proj_blocks(Y, param, merged):
    """Per point: the 3 x 3 projection Jacobian w.r.t. Y (rows uL, vL or sqrt 2 vL, uR) and the predictions (3 or 4 rows)."""
    f, cu, cv, b = param.f, param.cu, param.cv, param.base
    X, Yy, Z = Y
    n = Y.shape[1]
    Pj = np.zeros((n, 3, 3))
    Pj[:, 0, 0] = f / Z
    Pj[:, 0, 2] = -f * X / Z ** 2
    Pj[:, 1, 1] = f / Z
    Pj[:, 1, 2] = -f * Yy / Z ** 2
    Pj[:, 2, 0] = f / Z
    Pj[:, 2, 2] = -f * (X - b) / Z ** 2
    if merged:
        Pj[:, 1] *= RT2
    return Pj


def group_terms(W, g, trs, P):
    """For the tracks of group g at the state (trs, P): Jc (n, q, nc), Jx (n, q, 3), r (n, q) in the merged rows (the cost's
    gradient and Hessian are those of the full rows), cost (n,), and the mask of the rows that depend on the cameras."""
    param = W.param
    f, cu, cv, b = param.f, param.cu, param.cv, param.base
    so, eo = g["so"], g["eo"]
    n = P.shape[1]
    Rs, A = _chain(trs)
    Ws = [None] + [CR.omega(tr) for tr in trs]
    Ys, Qs = [P], [None]
    for j in range(1, eo + 1):
        q = Rs[j] @ Ys[-1]
        Qs.append(q)
        Ys.append(q + trs[j - 1][3:, None])
    blocks_c, blocks_x, res, cam = [], [], [], []
    cost = np.zeros(n)

    def cam_cols(Pj, j):
        Jc = np.zeros((n, 3, W.nc))
        for i in range(1, j + 1):
            M3 = Pj @ A[j][i]                                      # (n, 3, 3)
            D = np.zeros((n, 3, 6))
            for k in range(3):
                D[:, :, k] = np.cross(Ws[i][:, k][None, :], Qs[i].T)
            D[:, :, 3:] = np.eye(3)
            Jc[:, :, 6 * (i - 1):6 * i] = M3 @ D
        return Jc

    # frame s: pi_0 of Y_s against z0
    Y = Ys[so]
    Pj = _proj_blocks(Y, param, False)
    r0 = (g["z0"] - RR.project0(Y, param)).T
    cost += (r0 ** 2).sum(1)
    blocks_x.append(Pj @ A[so][0])
    blocks_c.append(cam_cols(Pj, so))
    res.append(r0)
    cam.append(so > 0)
    for j in range(so + 1, eo + 1):
        Y = Ys[j]
        pred = np.stack([f * Y[0] / Y[2] + cu, f * Y[1] / Y[2] + cv, f * (Y[0] - b) / Y[2] + cu, f * Y[1] / Y[2] + cv])
        r = (g["z"][:, j - so - 1, :].T - pred).T                  # (n, 4)
        cost += (r ** 2).sum(1)
        Pj = _proj_blocks(Y, param, True)
        blocks_x.append(Pj @ A[j][0])
        blocks_c.append(cam_cols(Pj, j))
        res.append(np.stack([r[:, 0], (r[:, 1] + r[:, 3]) / RT2, r[:, 2]], 1))
        cam.append(True)
    return (np.concatenate(blocks_c, 1), np.concatenate(blocks_x, 1), np.concatenate(res, 1), cost,
            np.repeat(np.array(cam), 3))


def total_cost(W, trs, Ps):
    return float(sum(group_terms(W, g, trs, P)[3].sum() for g, P in zip(W.groups, Ps)))


def normal_equations(W, trs, Ps, lam):
    """(S, s, per group (l, W~, y), ok): the reduced camera system with the diagonals of Hcc and of every Hpp multiplied by (1 + lam).
    ok is False when a point's Hpp_d or, for a track with s = a, its I - M'M (M = Jx of the camera rows x l^-T) fails the pivot test."""
    nc = W.nc
    Hcc = np.zeros((nc, nc))
    gc = np.zeros(nc)
    red = []
    WW = np.zeros((nc, nc))
    Wy = np.zeros(nc)
    for g, P in zip(W.groups, Ps):
        Jc, Jx, r, _c, cam = group_terms(W, g, trs, P)
        Hcc += np.einsum("nri,nrj->ij", Jc, Jc)
        gc += np.einsum("nri,nr->i", Jc, r)
        Hpp = np.einsum("nra,nrc->nac", Jx, Jx)
        gp = np.einsum("nra,nr->na", Jx, r)
        Hcp = np.einsum("nri,nrc->nic", Jc, Jx)
        d = np.arange(3)
        Hpp[:, d, d] *= 1.0 + lam
        if not RR.chol3_ok(Hpp):
            return None, None, None, False
        lc = np.linalg.cholesky(Hpp)
        if g["so"] == 0:
            Jxc = Jx[:, cam]
            Hxc = np.einsum("nra,nrc->nac", Jxc, Jxc)
            li = np.linalg.inv(lc)
            Q = np.eye(3) - li @ Hxc @ np.transpose(li, (0, 2, 1))
            if not RR.chol3_ok(Q):
                return None, None, None, False
        Wt = np.linalg.solve(lc, np.transpose(Hcp, (0, 2, 1)))    # (n, 3, nc) = l^-1 Hcp'
        y = np.linalg.solve(lc, gp[:, :, None])[:, :, 0]
        WW += np.einsum("nci,ncj->ij", Wt, Wt)
        Wy += np.einsum("nci,nc->i", Wt, y)
        red.append((lc, Wt, y))
    S = Hcc + lam * np.diag(np.diag(Hcc)) - WW
    return 0.5 * (S + S.T), gc - Wy, red, True


def chol_ok(A):
    """RR.chol_ok for any size."""
    return RR.chol_ok(A)


def _record(W, tr_t, tr_win, status, **kw):
    rec = dict(tr=np.array(tr_t, np.float64), cov=np.zeros((6, 6)), tr_win=np.zeros((4, 6)), sigma2=0.0, cost0=0.0, cost=0.0,
               gap=0.0, iters=0, status=status, len=0, n_points=0, n_rows=0, trace=[], slack=dict(RR.ZERO_SLACK))
    if tr_win is not None:
        rec["tr_win"][:len(tr_win)] = tr_win
    if W is not None:
        rec.update(len=W.len, n_points=W.n_points, n_rows=W.n_rows)
    rec.update(kw)
    return rec


def point_steps(red, dtr):
    """The points' steps (3, n) per group that go with the motions' step dtr."""
    out = []
    for lc, Wt, y in red:
        v = y - np.einsum("nci,i->nc", Wt, dtr)
        out.append(np.linalg.solve(np.transpose(lc, (0, 2, 1)), v[:, :, None])[:, :, 0].T)
    return out


def lm_step(W, trs, Ps, lam):
    """The step (dtr (nc), dX (3, n) per group) of the damped system at (trs, Ps), or None where the loop would leave with -2
    or -3."""
    S, s, red, good = normal_equations(W, trs, Ps, lam)
    if not good or not (np.all(np.isfinite(S)) and np.all(np.isfinite(s))) or not chol_ok(S):
        return None
    dtr = np.linalg.solve(S, s)
    return dtr, point_steps(red, dtr)


def step_sizes(step, Cinv, red0, pmax):
    """A step's size per compared quantity, as RR.step_sizes: tr_abs over every motion of the window (tr_win), tr_white frame t's
    motion whitened by its cov = Cinv^-1, the points relative to pmax and whitened by their undamped Hpp = l l' (red0: the
    undamped system's per-group terms)."""
    if step is None:
        return dict(RR.ZERO_SLACK)
    dtr, dXs = step
    white = [np.sqrt((np.einsum("nca,cn->na", lc, dX) ** 2).sum(1).max()) for (lc, _w, _y), dX in zip(red0, dXs)]
    return dict(tr_abs=float(np.abs(dtr).max()), tr_white=float(np.sqrt(dtr[-6:] @ Cinv @ dtr[-6:])),
                pts_rel=float(max(np.abs(dX).max() for dX in dXs) / pmax), pts_white=float(max(white)))


def window(frames, t, K, param, mode, sigma=None):
    """The record of frame t (a dict with the fields of viso_window_record, plus `trace`: the relative cost change (C_new - C) / C
    of every accept / reject decision, `points`: the final points per group, and `slack`: per quantity of step_sizes, the larger
    of the last accepted step and of one further step at the damping the loop would use next).  frames[j] is a Frame for j >= 1;
    frames[0] is not read."""
    if t == 0:
        return _record(None, np.zeros(6), None, 0)
    fr = frames[t]
    if fr.ok == 0:
        return _record(None, fr.tr, None, 0)
    if len(fr.Lp) < 6:
        return _record(None, fr.tr, None, -1)
    a = anchor(frames, t, K)
    W = Window(frames, a, t, param)
    tr_in = W.tr0.copy()
    denom = W.n_rows - 3 * W.n_points - W.nc
    if denom <= 0:
        return _record(W, fr.tr, tr_in, -1)
    trs = tr_in.copy()
    Ps = W.start_points()
    with np.errstate(all="ignore"):
        C = total_cost(W, trs, Ps)
        C0 = C
        lam, acc, rej = LAMBDA0, 0, 0
        trace, last = [], None
        if not np.isfinite(C):
            return _record(W, fr.tr, tr_in, -3)
        while C != 0.0:
            S, s, red, good = normal_equations(W, trs, Ps, lam)
            if good and not (np.all(np.isfinite(S)) and np.all(np.isfinite(s))):
                return _record(W, fr.tr, tr_in, -3)
            if not good or not chol_ok(S):
                return _record(W, fr.tr, tr_in, -2)
            dtr = np.linalg.solve(S, s)
            dXs = point_steps(red, dtr)
            Pn = [P + dX for P, dX in zip(Ps, dXs)]
            trn = trs + dtr.reshape(-1, 6)
            Cn = total_cost(W, trn, Pn)
            trace.append((Cn - C) / C)
            if Cn < C:
                acc += 1
                rej = 0
                lam = max(lam / 10.0, LAMBDA_MIN)
                stop = C - Cn <= REL_TOL * C or Cn == 0.0 or acc == MAX_ACCEPT
                trs, Ps, C = trn, Pn, Cn
                last = (dtr, dXs)
                if stop:
                    break
            else:
                lam *= 10.0
                rej += 1
                if rej == MAX_REJECT:
                    break
        S, s, red0, good = normal_equations(W, trs, Ps, 0.0)
        if good and not (np.all(np.isfinite(S)) and np.all(np.isfinite(s))):
            return _record(W, fr.tr, tr_in, -3)
        if not good or not chol_ok(S):
            return _record(W, fr.tr, tr_in, -2)
        s2 = float(sigma) ** 2 if mode == 2 else C / denom
        Si = np.linalg.inv(S)
        Stt = Si[-6:, -6:]
        cov = s2 * 0.5 * (Stt + Stt.T)
        gap = float(s @ Si @ s) / s2 if s2 > 0 else 0.0
        if not (np.all(np.isfinite(cov)) and np.isfinite(gap) and np.all(np.isfinite(trs))):
            return _record(W, fr.tr, tr_in, -3)
        further = lm_step(W, trs, Ps, lam) if C != 0.0 else None
        Cinv = np.linalg.inv(0.5 * (Stt + Stt.T)) / max(s2, 1e-300)
        pmax = float(max(np.abs(P).max() for P in Ps))
        a, b = step_sizes(last, Cinv, red0, pmax), step_sizes(further, Cinv, red0, pmax)
        slack = {k: max(a[k], b[k]) for k in a}
    return _record(W, trs[-1], trs, 1, cov=cov, sigma2=s2, cost0=C0, cost=C, gap=gap, iters=acc, trace=trace, points=Ps,
                   window=W, slack=slack)


def records(frames, K, param, mode, sigma=None):
    return [window(frames, t, K, param, mode, sigma) for t in range(len(frames))]


def dense_hessian(W, trs, Ps):
    """The undamped Gauss-Newton Hessian of the full cost over (tr_{a+1..t}, every track's X in group order) and its gradient."""
    nc = W.nc
    n = sum(P.shape[1] for P in Ps)
    Jrows, rs = [], []
    col = nc
    for g, P in zip(W.groups, Ps):
        Jc, Jx, r, _c, _m = group_terms(W, g, trs, P)
        for k in range(P.shape[1]):
            J = np.zeros((Jc.shape[1], nc + 3 * n))
            J[:, :nc] = Jc[k]
            J[:, col:col + 3] = Jx[k]
            Jrows.append(J)
            rs.append(r[k])
            col += 3
    J = np.concatenate(Jrows, 0)
    r = np.concatenate(rs)
    return J.T @ J, J.T @ r


def frames_from_batch(b):
    """[None, Frame(1), ..., Frame(nf - 1)] from a Batch's last run (points, circle rows, pose)."""
    out = [None]
    for t in range(1, b.nf):
        X, obs = b.points(t)
        circ, _pcl = b.circle(t)
        ok, tr, inl = b.pose(t)
        out.append(Frame(X, obs, circ[:, [0, 2]], tr, ok, inl))
    return out
