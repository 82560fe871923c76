"""numpy restatement of the pose-graph optimiser (include/viso_hip.h, "pose graph"): Exp, Log and the exact Jacobians of SE(3) in
the tangent order (phi, rho), the dense normal equations, the Levenberg-Marquardt step by a dense solve and by the
chain-plus-low-rank form the device uses, and the loop.  A graph is (poses [n][4][4], fixed [n], ij [m][2], Z [m][4][4],
info [m][6][6]).  Everything is float64 and loops over edges in edge-index order unless an order is passed in."""
import numpy as np

SERIES_THETA2 = 1e-2      # below it the coefficients are their series, five terms each
LAMBDA0, LAMBDA_MIN = 1e-4, 1e-12
ACCEPT_SLACK = 2.0 ** -40
PIVOT = 1e-12

_FACT = [1.0]
for _k in range(1, 16):
    _FACT.append(_FACT[-1] * _k)


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def _series(th2, off, weight=lambda k: 1.0):
    s, p = 0.0, 1.0
    for k in range(5):
        s += (-1.0) ** k * weight(k) * p / _FACT[2 * k + off]
        p *= th2
    return s


def coeffs(th2):
    """a = sin t / t, b = (1 - cos t) / t^2, c1 = (t - sin t) / t^3, c2 = (t^2 + 2 cos t - 2) / (2 t^4),
    c3 = (2 t - 3 sin t + t cos t) / (2 t^5), cp = (1 - a / (2 b)) / t^2, at t^2 = th2."""
    if th2 < SERIES_THETA2:
        a, b, c1, c2 = _series(th2, 1), _series(th2, 2), _series(th2, 3), _series(th2, 4)
        c3 = _series(th2, 5, lambda k: k + 1.0)
        cp = 1.0 / 12 + th2 * (1.0 / 720 + th2 * (1.0 / 30240 + th2 * (1.0 / 1209600 + th2 / 47900160)))
        return a, b, c1, c2, c3, cp
    t = np.sqrt(th2)
    s, c = np.sin(t), np.cos(t)
    a, b = s / t, (1.0 - c) / th2
    return (a, b, (t - s) / (th2 * t), (th2 + 2.0 * c - 2.0) / (2.0 * th2 * th2), (2.0 * t - 3.0 * s + t * c) / (2.0 * th2 * th2 * t),
            (1.0 - a / (2.0 * b)) / th2)


def exp_se3(xi):
    phi, rho = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    a, b, c1 = coeffs(phi @ phi)[:3]
    K = hat(phi)
    K2 = K @ K
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + a * K + b * K2
    T[:3, 3] = (np.eye(3) + b * K + c1 * K2) @ rho
    return T


def log_se3(T):
    R, t = T[:3, :3], T[:3, 3]
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt(v @ v)
    theta = np.arctan2(s, 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0))
    th2 = theta * theta
    a, _, _, _, _, cp = coeffs(th2)
    phi = v / a
    K = hat(phi)
    rho = (np.eye(3) - 0.5 * K + cp * (K @ K)) @ t
    return np.concatenate([phi, rho])


def inv_se3(T):
    out = np.eye(4)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    return out


def adj(T):
    R, t = T[:3, :3], T[:3, 3]
    A = np.zeros((6, 6))
    A[:3, :3] = R
    A[3:, 3:] = R
    A[3:, :3] = hat(t) @ R
    return A


def jr_inv(xi):
    """J_r^-1(xi) in (phi, rho) order: [[A, 0], [-A Q A, A]], A = J_l,SO3(-phi)^-1, Q = Q(-rho, -phi)."""
    phi, rho = -np.asarray(xi[:3], float), -np.asarray(xi[3:], float)
    th2 = phi @ phi
    _, _, c1, c2, c3, cp = coeffs(th2)
    P, Rh = hat(phi), hat(rho)
    A = np.eye(3) - 0.5 * P + cp * (P @ P)
    PR, RP = P @ Rh, Rh @ P
    PRP = PR @ P
    Q = (0.5 * Rh + c1 * (PR + RP + PRP) + c2 * (P @ PR + RP @ P - 3.0 * PRP) + c3 * (PRP @ P + P @ PRP))
    J = np.zeros((6, 6))
    J[:3, :3] = A
    J[3:, 3:] = A
    J[3:, :3] = -A @ Q @ A
    return J


def edge_terms(poses, i, j, Z):
    """r, J_i (None for a prior), J_j of one edge."""
    M = poses[j] if i < 0 else inv_se3(poses[i]) @ poses[j]
    r = log_se3(inv_se3(Z) @ M)
    Jj = jr_inv(r)
    return r, (None if i < 0 else -Jj @ adj(inv_se3(M))), Jj


def is_long(i, j):
    return i >= 0 and abs(i - j) != 1


def cost(poses, ij, Z, info, order=None):
    F = 0.0
    for e in (range(len(ij)) if order is None else order):
        r = edge_terms(poses, ij[e][0], ij[e][1], Z[e])[0]
        F += 0.5 * r @ info[e] @ r
    return F


def linearize_dense(poses, fixed, ij, Z, info, order=None):
    """cost, g [n][6] and dense H [6n][6n]; rows and columns of fixed nodes stay zero."""
    n = len(poses)
    g, H, F = np.zeros((n, 6)), np.zeros((6 * n, 6 * n)), 0.0
    for e in (range(len(ij)) if order is None else order):
        i, j = int(ij[e][0]), int(ij[e][1])
        r, Ji, Jj = edge_terms(poses, i, j, Z[e])
        F += 0.5 * r @ info[e] @ r
        ends = [(a, J) for a, J in ((i, Ji), (j, Jj)) if a >= 0 and not fixed[a]]
        for a, Ja in ends:
            g[a] += Ja.T @ info[e] @ r
            for b, Jb in ends:
                H[6 * a:6 * a + 6, 6 * b:6 * b + 6] += Ja.T @ info[e] @ Jb
    return F, g, H


def _free_index(fixed):
    return np.concatenate([np.arange(6 * k, 6 * k + 6) for k in range(len(fixed)) if not fixed[k]] or [np.zeros(0, int)]).astype(int)


def step_dense(H, g, fixed, lam):
    """delta [n][6] of (H + lam diag H) delta = -g over the free nodes."""
    idx = _free_index(fixed)
    out = np.zeros(g.size)
    if idx.size:
        Hf = H[np.ix_(idx, idx)]
        out[idx] = np.linalg.solve(Hf + lam * np.diag(np.diag(Hf)), -g.reshape(-1)[idx])
    return out.reshape(-1, 6)


def chol6(S, orig):
    L = np.zeros((6, 6))
    for c in range(6):
        d = S[c, c] - L[c, :c] @ L[c, :c]
        if not d > PIVOT * orig[c]:
            return None
        L[c, c] = np.sqrt(d)
        for p in range(c + 1, 6):
            L[p, c] = (S[p, c] - L[p, :c] @ L[c, :c]) / L[c, c]
    return L


def step_chain(poses, fixed, ij, Z, info, lam):
    """The same step by the form the device uses: T = chain edges + damping (block tridiagonal), the long edges as U U',
    delta = y - W (I + U' W)^-1 U' y.  Returns delta [n][6], or None when a pivot fails."""
    n = len(poses)
    D, E, g, dH = np.zeros((n, 6, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6)), np.zeros((n, 6))
    long_edges = [e for e in range(len(ij)) if is_long(int(ij[e][0]), int(ij[e][1]))]
    U = np.zeros((6 * n, 6 * len(long_edges)))
    for e in range(len(ij)):
        i, j = int(ij[e][0]), int(ij[e][1])
        r, Ji, Jj = edge_terms(poses, i, j, Z[e])
        C = np.linalg.cholesky(info[e])
        B = {a: J.T @ C for a, J in ((i, Ji), (j, Jj)) if a >= 0 and not fixed[a]}
        w = C.T @ r
        for a, Ba in B.items():
            g[a] += Ba @ w
            dH[a] += np.sum(Ba * Ba, axis=1)
            if e in long_edges:
                U[6 * a:6 * a + 6, 6 * long_edges.index(e):6 * long_edges.index(e) + 6] = Ba
            else:
                D[a] += Ba @ Ba.T
        if e not in long_edges and len(B) == 2:
            lo = min(i, j)
            E[lo] += B[lo + 1] @ B[lo].T          # block (lo + 1, lo)
    for k in range(n):
        if fixed[k]:
            D[k] = np.eye(6)
        else:
            D[k] += lam * np.diag(dH[k])
    rhs = np.concatenate([U, -g.reshape(-1, 1)], axis=1).reshape(n, 6, -1)
    Li, Fk = np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
    for k in range(n):                               # block-tridiagonal Cholesky
        S = D[k] - (Fk[k - 1] @ Fk[k - 1].T if k else 0.0)
        L = chol6(S, np.diag(D[k]))
        if L is None:
            return None
        Li[k] = np.linalg.inv(L)
        Fk[k] = E[k] @ Li[k].T
    X = np.zeros_like(rhs)
    for k in range(n):                               # forward, then backward
        X[k] = Li[k] @ (rhs[k] - (Fk[k - 1] @ X[k - 1] if k else 0.0))
    for k in range(n - 1, -1, -1):
        X[k] = Li[k].T @ (X[k] - (Fk[k].T @ X[k + 1] if k + 1 < n else 0.0))
    X = X.reshape(6 * n, -1)
    W, y = X[:, :-1], X[:, -1]
    if W.shape[1]:
        S = np.eye(W.shape[1]) + U.T @ W
        if chol6_general(S) is None:
            return None
        y = y - W @ np.linalg.solve(S, U.T @ y)
    out = y.reshape(n, 6).copy()
    out[np.asarray(fixed, bool)] = 0.0
    return out


def chol6_general(S):
    L = np.zeros_like(S)
    for c in range(len(S)):
        d = S[c, c] - L[c, :c] @ L[c, :c]
        if not d > PIVOT * S[c, c]:
            return None
        L[c, c] = np.sqrt(d)
        L[c + 1:, c] = (S[c + 1:, c] - L[c + 1:, :c] @ L[c, :c]) / L[c, c]
    return L


def retract(poses, fixed, delta):
    return np.array([P if fixed[k] else P @ exp_se3(delta[k]) for k, P in enumerate(poses)])


def optimize(poses, fixed, ij, Z, info, max_iters=50, eps_step=1e-10, chain=False):
    """The loop of "One iteration": poses, report dict, trace [[F, F', lambda, max|delta|, accepted]]."""
    poses = np.array(poses, float)
    F, g, H = linearize_dense(poses, fixed, ij, Z, info)
    rep = dict(status=2, iters=0, cost_initial=F, cost_final=F, last_step=0.0, n_rejected=0,
               n_long=sum(is_long(int(a), int(b)) for a, b in ij))
    lam, trace = LAMBDA0, []
    for it in range(max_iters):
        d = step_chain(poses, fixed, ij, Z, info, lam) if chain else step_dense(H, g, fixed, lam)
        rep["iters"] = it + 1
        step = float(np.abs(d).max())
        rep["last_step"] = step
        if step <= eps_step:
            trace.append([F, F, lam, step, 0.0])
            rep["status"] = 1
            break
        trial = retract(poses, fixed, d)
        Ft = cost(trial, ij, Z, info)
        ok = Ft <= F * (1.0 + ACCEPT_SLACK)
        trace.append([F, Ft, lam, step, float(ok)])
        if ok:
            poses, lam = trial, max(lam * 0.1, LAMBDA_MIN)
            F, g, H = linearize_dense(poses, fixed, ij, Z, info)
        else:
            lam *= 10.0
            rep["n_rejected"] += 1
    rep["cost_final"], rep["lambda"] = F, lam
    return poses, rep, np.array(trace).reshape(-1, 5)


# ---- synthetic graphs of the tests and of tools/posegraph_bench.py -----------------------------------------------------------------
def random_pose(rng, rot=0.3, trans=1.0):
    return exp_se3(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3)]))


def random_info(rng, scale=1.0):
    A = rng.normal(size=(6, 6))
    return scale * (A @ A.T + 6.0 * np.eye(6))


def loop_truth(n, radius=10.0):
    """n poses around a circle, looking along the tangent, with a slow roll."""
    out = []
    for k in range(n):
        a = 2.0 * np.pi * k / max(n, 1)
        T = exp_se3(np.array([0.05 * np.sin(3 * a), a, 0.03 * np.cos(2 * a), 0, 0, 0]))
        T[:3, 3] = [radius * np.cos(a), 0.2 * np.sin(2 * a), radius * np.sin(a)]
        out.append(T)
    return np.array(out)


def make_graph(rng, n, n_long, noise=0.0, n_priors=1, fixed=(0,), reversed_every=0, duplicates=0, drift=0.02):
    """A chain of n poses around a loop with n_long long edges, measured with `noise` (tangent sigma), started from a chain that
    drifts, its first pose included: residuals of 0.1 and more.  (The loop's radius is 10, so a residual carries an absolute error
    of some 1e-15 from the products in front of Log; the cost of a graph whose residuals are all 1e-2 is known to 1e-13 of itself
    and no better, in this restatement as anywhere else in doubles.)  Returns (poses0, fixed, ij, Z, info, truth)."""
    truth = loop_truth(n)
    ij, Z, info = [], [], []

    def add(i, j):
        M = truth[j] if i < 0 else inv_se3(truth[i]) @ truth[j]
        ij.append((i, j))
        Z.append(M @ exp_se3(rng.normal(0, noise, 6)) if noise else M)
        info.append(random_info(rng, 100.0))

    for k in range(n - 1):
        if reversed_every and k % reversed_every == 1:
            add(k + 1, k)
        else:
            add(k, k + 1)
    for m in range(n_long):
        i = int(rng.integers(0, max(n - 2, 1)))
        j = int(rng.integers(i + 2, n)) if n > 2 else i
        if m % 2:
            i, j = j, i
        add(i, j)
    for m in range(duplicates):
        add(*ij[int(rng.integers(0, n - 1))])   # of a chain edge: the number of long edges stays n_long
    for m in range(n_priors):
        add(-1, int(rng.integers(0, n)) if m else n - 1)
    fx = np.zeros(n, np.int32)
    for k in fixed:
        fx[k] = 1
    poses0 = [truth[0] @ exp_se3(rng.normal(0, 10.0 * drift, 6))]   # (a fixed first node is put back below)
    for k in range(1, n):
        poses0.append(poses0[-1] @ inv_se3(truth[k - 1]) @ truth[k] @ exp_se3(rng.normal(0, drift, 6)))
    poses0 = np.array(poses0)
    for k in fixed:
        poses0[k] = truth[k]
    return poses0, fx, np.array(ij, np.int32).reshape(-1, 2), np.array(Z), np.array(info), truth


def make_structured(rng, n, edges, fixed=(), noise=0.01, start=0.05):
    """A graph over loop_truth(n) with exactly the edges listed, in that order ((i, j); i = -1 is a prior on j), measured with
    `noise`, the fixed nodes at their truth and every other node started `start` (tangent sigma) off its own truth.  The structure
    -- gaps in the chain, reversed and double edges, which nodes are fixed -- is the caller's list, nothing is drawn.  Returns what
    make_graph returns."""
    truth = loop_truth(n)
    Z, info = [], []
    for i, j in edges:
        M = truth[j] if i < 0 else inv_se3(truth[i]) @ truth[j]
        Z.append(M @ exp_se3(rng.normal(0, noise, 6)) if noise else M)
        info.append(random_info(rng, 100.0))
    fx = np.zeros(n, np.int32)
    fx[list(fixed)] = 1
    poses0 = np.array([truth[k] if fx[k] else truth[k] @ exp_se3(rng.normal(0, start, 6)) for k in range(n)])
    return poses0, fx, np.array(edges, np.int32).reshape(-1, 2), np.array(Z), np.array(info), truth

