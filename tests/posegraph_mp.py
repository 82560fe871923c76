"""A 60-digit reference of the pose graph's SE(3) math (include/viso_hip.h, "pose graph": "Exp and Log", "Jacobians"), for the CPU
tests only: mpmath at mp.dps = 60.  Exp is the header's closed form, which at 60 digits cancels nothing for theta >= 1e-9, so there
is neither a series nor a threshold (and mpmath's matrix exponential of the twist agrees, which test_posegraph_cases_cpu.py checks);
Log takes phi from the header's definition and rho by solving V(phi) rho = t, so no closed form of cp is used; J_i and J_j are
central differences of r = Log(Z^-1 P_i^-1 P_j) under the right perturbation P Exp(d) at h = 1e-20 (truncation h^2 = 1e-40, rounding
1e-60 / h = 1e-40).  Nothing here shares a formula for Q, c2, c3 or cp with the kernel or with tests/posegraph_ref.py.  Matrices go
in as the float64 values the device gets, exactly; as the header says, the first three rows are taken as rigid, so an inverse is
[R' | -R' t]."""
import mpmath as mp
import numpy as np

DPS = 60
H = mp.mpf(10) ** -20


def _mat(A):
    A = np.asarray(A, np.float64)
    return mp.matrix([[mp.mpf(float(x)) for x in row] for row in A])


def _np(A):
    return np.array([[float(A[i, j]) for j in range(A.cols)] for i in range(A.rows)])


def _hat(v):
    return mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])


def _pose(R, t):
    T = mp.eye(4)
    T[0:3, 0:3] = R
    for a in range(3):
        T[a, 3] = t[a]
    return T


def _exp(xi):
    phi, rho = mp.matrix(xi[0:3]), mp.matrix(xi[3:6])
    th2 = sum(x * x for x in phi)
    K = _hat(phi)
    K2 = K * K
    if th2 == 0:
        return _pose(mp.eye(3), rho)
    th = mp.sqrt(th2)
    a, b, c1 = mp.sin(th) / th, (1 - mp.cos(th)) / th2, (th - mp.sin(th)) / (th2 * th)
    return _pose(mp.eye(3) + a * K + b * K2, (mp.eye(3) + b * K + c1 * K2) * rho)


def _inv(T):
    Rt = T[0:3, 0:3].T
    return _pose(Rt, -(Rt * T[0:3, 3]))


def _log(T):
    R, t = T[0:3, 0:3], T[0:3, 3]
    v = mp.matrix([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    s = mp.sqrt(sum(x * x for x in v))
    th = mp.atan2(s, (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2)
    if th == 0:
        return [mp.mpf(0)] * 3 + list(t)
    phi = v * (th / mp.sin(th))
    K = _hat(phi)
    V = mp.eye(3) + ((1 - mp.cos(th)) / th ** 2) * K + ((th - mp.sin(th)) / th ** 3) * (K * K)
    return list(phi) + list(mp.lu_solve(V, t))


def _residual(Pi, Pj, Z):
    M = Pj if Pi is None else _inv(Pi) * Pj
    return mp.matrix(_log(_inv(Z) * M))


def exp_se3(xi):
    """Exp(xi) [4][4] as float64, rounded once from 60 digits."""
    with mp.workdps(DPS):
        return _np(_exp([mp.mpf(float(x)) for x in xi]))


def self_check(xi):
    """(max |Exp(xi) - expm(twist)|, max |Log(Exp(xi)) - xi|) at 60 digits: mpmath's matrix exponential of the 4 x 4 twist
    [[K, rho], [0, 0]] knows no closed form at all."""
    with mp.workdps(DPS):
        x = [mp.mpf(float(v)) for v in xi]
        A = mp.zeros(4)
        A[0:3, 0:3] = _hat(x[0:3])
        for a in range(3):
            A[a, 3] = x[3 + a]
        D = _exp(x) - mp.expm(A)
        back = mp.matrix(_log(_exp(x))) - mp.matrix(x)
        return float(max(abs(D[i, j]) for i in range(4) for j in range(4))), float(max(abs(v) for v in back))


def log_se3(T):
    with mp.workdps(DPS):
        return np.array([float(x) for x in _log(_mat(T))])


def edge_terms(Pi, Pj, Z):
    """r [6], J_i [6][6] (None for a prior: Pi None), J_j [6][6] of one edge, float64 rounded once from 60 digits."""
    with mp.workdps(DPS):
        Pi, Pj, Z = None if Pi is None else _mat(Pi), _mat(Pj), _mat(Z)
        r = _residual(Pi, Pj, Z)
        out = []
        for side in (0, 1):
            if side == 0 and Pi is None:
                out.append(None)
                continue
            J = mp.zeros(6)
            for k in range(6):
                d = [mp.mpf(0)] * 6
                d[k] = H
                Ep, Em = _exp(d), _exp([-x for x in d])
                if side == 0:
                    rp, rm = _residual(Pi * Ep, Pj, Z), _residual(Pi * Em, Pj, Z)
                else:
                    rp, rm = _residual(Pi, Pj * Ep, Z), _residual(Pi, Pj * Em, Z)
                for m in range(6):
                    J[m, k] = (rp[m] - rm[m]) / (2 * H)
            out.append(_np(J))
        return np.array([float(x) for x in r]), out[0], out[1]
