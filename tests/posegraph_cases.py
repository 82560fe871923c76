"""The cases of tests/test_posegraph_cases_cpu.py and tests/test_gpu_posegraph_edges.py, built once and shared: single edges at
residual rotations on both sides of the series threshold and up to 3 rad (the SE(3) math against tests/posegraph_mp.py's 60
digits, then the device edge by edge), graphs at the seams of pg_dense_kernel and pg_cost_kernel, chains with gaps and fixed
nodes written down node by node, the graph whose first trial is rejected and the chain whose only anchor is too weak to factor.
Nothing here touches a device or mpmath."""
import numpy as np

import posegraph_ref as R

# ---- A. single edges -----------------------------------------------------------------------------------------------------------------
# The restatement (float64) against 60 digits: the worst absolute error of r, J_i, J_j (an edge and a prior) and Exp over the largest
# entry of the quantity, per case of math_cases().  Measured (tests/test_posegraph_cases_cpu.py prints every figure):
#   theta     unit translations: r, J_i, J_j           poses 500 m out: r, J_i, J_j           (the larger of the edge's and the prior's)
#   1e-9      1.9e-16  1.4e-16  2.2e-16                1.9e-14  3.6e-15  1.2e-14
#   1e-4      1.7e-16  1.1e-16  1.1e-16                6.4e-14  7.1e-15  3.4e-14
#   0.05      3.5e-16  1.2e-16  1.1e-16                4.4e-14  1.5e-14  2.9e-14
#   0.0999    1.9e-16  2.4e-16  3.3e-16                1.5e-14  2.9e-15  1.1e-14
#   0.1001    1.0e-14  6.6e-15  6.7e-15                2.3e-14  2.0e-14  2.5e-14
#   0.3       1.3e-15  1.0e-15  1.1e-15                5.4e-14  2.8e-14  3.0e-14
#   0.7       2.0e-16  4.2e-16  5.6e-16                3.2e-14  7.4e-15  1.8e-14
#   1.0       3.5e-16  3.2e-16  5.8e-16                4.2e-14  4.7e-15  1.9e-14
#   2.0       2.5e-16  3.6e-16  5.5e-16                3.0e-14  1.1e-14  2.5e-14
#   3.0       1.2e-15  4.4e-15  9.6e-15                2.7e-14  1.4e-14  2.9e-14
# Exp(xi) of every case: 0 .. 5.2e-16, held to MATH_BOUND at either scale (a tangent vector has no 500 m in it).
# The bounds are what float64 gives these formulas, not what any device gives.  With unit translations the worst is just above the
# switch, where the closed forms of c2, c3 and cp cancel (the header's 1e-16 / theta^4 is 1e-12 of each at theta = 0.1, on terms
# of a hundredth of the largest entry: 1e-14), and at 3 rad, where a = sin(theta) / theta is 0.047 and phi = v / a carries v's
# rounding 21 times over.  2^-45 = 2.8e-14 covers both with a factor of 3.  500 m out the restatement forms P_i^-1 P_j as a matrix
# product, -R_i' t_i + R_i' t_j: two numbers of 500 rounded at 2^-53 each and the three products and two sums behind each, some
# four roundings of 5.6e-14 in a translation of order one, so 2^-42 = 2.3e-13.  (The device subtracts t_j - t_i first, which
# rounds less; its figures are in tests/test_gpu_posegraph_edges.py.)
MATH_BOUND = 2.0 ** -45
MATH_BOUND_FAR = 2.0 ** -42
# (0.7: between the switch and 1 rad five terms of the series are 1e-9 short, so a switch moved up shows there)
MATH_THETAS = (1e-9, 1e-4, 0.05, 0.0999, 0.1001, 0.3, 0.7, 1.0, 2.0, 3.0)
FAR = np.array([310.0, -12.0, 395.0])      # |FAR| = 502 m: where a KITTI trajectory is after a few minutes
MIN_COMPONENT = 0.05                       # every component of every residual, where |phi| = theta allows it (see math_cases)
_math = []


def _spread_direction(rng, spread):
    d = rng.choice([-1.0, 1.0], 3) * (1.0 + spread * rng.uniform(-1.0, 1.0, 3))
    return d / np.linalg.norm(d)


def math_cases():
    """[dict(name, theta, far, bound, Pi, Pj, Z, Zp, xi)]: an edge (Pi, Pj, Z) whose residual is xi up to rounding, |xi[:3]| = theta, and a
    prior Zp on Pj with the same residual.  The probes weigh row m of a Jacobian by r_m, so no component of a residual is small:
    every |rho_m| is in 0.3 .. 1.5, and every |phi_m| >= 0.05 from theta = 0.0999 on.  Below that no rotation has three components
    of 0.05 (|phi| = theta < 0.05 sqrt 3): there every |phi_m| >= 0.5 theta, the rotation rows carry what weight they can, and A
    and Q are still probed through the translation rows [-A Q A, A]."""
    if not _math:
        for far in (False, True):
            for t, theta in enumerate(MATH_THETAS):
                rng = np.random.default_rng(1000 * far + t)
                phi = theta * _spread_direction(rng, 0.05 if theta < 0.3 else 0.5)
                rho = rng.choice([-1.0, 1.0], 3) * rng.uniform(0.3, 1.5, 3)
                xi = np.concatenate([phi, rho])
                Pi, Pj = R.random_pose(rng), R.random_pose(rng)
                if far:
                    Pi[:3, 3] += FAR
                    Pj[:3, 3] += FAR
                back = R.inv_se3(R.exp_se3(xi))
                _math.append(dict(name=f"theta{theta:g}_{'far' if far else 'unit'}", theta=theta, far=far, Pi=Pi, Pj=Pj,
                                  bound=MATH_BOUND_FAR if far else MATH_BOUND,
                                  Z=R.inv_se3(Pi) @ Pj @ back, Zp=Pj @ back, xi=xi))
    return _math


def probe_infos():
    """I, and I + 99 e_m e_m' for m = 0 .. 5: the second kind makes r_m times row m of J nearly all of the gradient."""
    out = [np.eye(6)]
    for m in range(6):
        O = np.eye(6)
        O[m, m] = 100.0
        out.append(O)
    return out


PROBE_SHAPES = ("j_free", "i_free", "prior")
_probes = {}


def probe_graph(shape):
    """Every (case, information matrix) pair as two nodes 2c, 2c + 1 of one graph with no edge between pairs ("prior": one node c):
    j_free is [P_i fixed, P_j free] with the edge (2c, 2c + 1), i_free is [P_i free, P_j fixed], prior is P_j with the prior Zp.
    Every free node is a run of its own.  Returns (poses, fixed, ij, Z, info, free, bound): free[c] is the free node of pair c and
    bound[c] its case's bound."""
    if shape not in _probes:
        poses, fixed, ij, Z, info, free, bound = [], [], [], [], [], [], []
        for case in math_cases():
            for O in probe_infos():
                k = len(poses)
                if shape == "prior":
                    poses.append(case["Pj"]); fixed.append(0); ij.append((-1, k)); Z.append(case["Zp"]); free.append(k)
                else:
                    poses += [case["Pi"], case["Pj"]]
                    fixed += [1, 0] if shape == "j_free" else [0, 1]
                    ij.append((k, k + 1)); Z.append(case["Z"]); free.append(k + 1 if shape == "j_free" else k)
                info.append(O)
                bound.append(case["bound"])
        _probes[shape] = (np.array(poses), np.array(fixed, np.int32), np.array(ij, np.int32), np.array(Z), np.array(info), np.array(free),
                          np.array(bound))
    return _probes[shape]


# ---- C. the seams of the solver --------------------------------------------------------------------------------------------------------
# name -> (n_poses, n_long, the factor on the long edges' information): R.make_graph(rng, n, L, noise=0.01), info symmetrised.
# 140 nodes have 139 chain edges and one prior, so L = 171 makes 311 edges: pg_cost_kernel's second trip.
SEAMS = {
    "n140_L16": (140, 16, 1.0),          # m = 96 = 3 x 32: the dense factor's last block is full
    "n140_L170": (140, 170, 1.0),        # m = 1020: the last order at which every i += 1024 loop makes one trip
    "n140_L171": (140, 171, 1.0),        # m = 1026: the load of v and the forward solve take a second trip
    "n140_L177": (140, 177, 1.0),        # m = 1062: c0 = 0 has 1030 rows below its block, a second trip there too
    "n140_L256": (140, 256, 1.0),        # m = 1536 = 48 x 32: the cap, a full last block
    "n65_L11_strong": (65, 11, 1e4),     # loop closures far tighter than the odometry
}
_graphs = {}


def _symmetric(g):
    return g[:4] + (0.5 * (g[4] + g[4].transpose(0, 2, 1)),) + g[5:]


def seam_graph(name):
    if name not in _graphs:
        n, L, strong = SEAMS[name]
        g = _symmetric(R.make_graph(np.random.default_rng(sum(map(ord, name))), n, L, noise=0.01))
        for e, (i, j) in enumerate(g[2]):
            if R.is_long(int(i), int(j)):
                g[4][e] *= strong
        _graphs[name] = g
    return _graphs[name]


def runs_of(fixed, ij):
    """The runs of T as the header's "Refusals" defines them: [(first, one past last, anchors)] over the free nodes joined by chain
    edges, a fixed node or a missing chain edge cutting a run.  anchors: the run's anchoring edges as (kind, edge index), kind
    "prior", "fixed" (a chain edge (k, k + 1) to a fixed node) or "fixed_reversed" ((k + 1, k))."""
    n = len(fixed)
    link, anchor = np.zeros(n, bool), [[] for _ in range(n)]
    for e, (i, j) in enumerate(ij):
        i, j = int(i), int(j)
        if R.is_long(i, j):
            continue
        kind = "fixed" if j == i + 1 else "fixed_reversed"
        if i < 0:
            anchor[j].append(("prior", e))
        elif fixed[i] and not fixed[j]:
            anchor[j].append((kind, e))
        elif fixed[j] and not fixed[i]:
            anchor[i].append((kind, e))
        elif not fixed[i] and not fixed[j]:
            link[min(i, j)] = True
    out, k = [], 0
    while k < n:
        if fixed[k]:
            k += 1
            continue
        k1 = k
        while k1 + 1 < n and not fixed[k1 + 1] and link[k1]:
            k1 += 1
        out.append((k, k1 + 1, [a for node in anchor[k:k1 + 1] for a in node]))
        k = k1 + 1
    return out


def _chain(n, gaps=(), reverse=()):
    """The chain edges (k, k + 1) of n nodes but those in `gaps`; the ones in `reverse` as (k + 1, k)."""
    return [((k + 1, k) if k in reverse else (k, k + 1)) for k in range(n - 1) if k not in gaps]


# Chains with gaps, written down.  70 nodes; fixed 20, 21 (adjacent) and 50; no chain edge 10|11, 11|12, 40|41, 68|69; the chain
# edges at 21|22, 30|31 and 50|51 are reversed.  The runs and what anchors each:
#   0 .. 10   (starts at node 0)       a prior on 5
#   11        (length one, both chain edges missing)   two priors on 11
#   12 .. 19                            the chain edge (19, 20) to the fixed 20 only
#   22 .. 40                            the reversed chain edge (22, 21) to the fixed 21 only
#   41 .. 49                            a prior on 41, and the chain edge (49, 50) to the fixed 50
#   51 .. 68                            the reversed chain edge (51, 50) to the fixed 50 only
#   69        (length one, at node n - 1)   a prior on 69
# Long edges: (3, 30) joins two runs; (20, 45) has its i end fixed, (33, 50) its j end, (20, 50) both (cost only, its six columns
# of U are zero); (8, 60) and (60, 8) are two on one pair, one reversed; (11, 69) joins the two runs of length one; (0, 69) the
# two ends of the array; (14, 16) lies inside a run.
SHAPES_A = dict(
    n=70, fixed=(20, 21, 50), gaps=(10, 11, 40, 68), reverse=(21, 30, 50), priors=(5, 11, 11, 41, 69),
    long=((3, 30), (20, 45), (33, 50), (20, 50), (8, 60), (60, 8), (11, 69), (0, 69), (14, 16)),
    runs=((0, 11), (11, 12), (12, 20), (22, 41), (41, 50), (51, 69), (69, 70)))
# 12 nodes, the last one fixed; fixed 5, 6 (adjacent) and 11; no chain edge 2|3; (11, 10) reversed.  Runs: 0 .. 2 with two priors on
# node 1; 3, 4 with the chain edge (4, 5); 7 .. 10 with the chain edges (6, 7) and the reversed (11, 10) to the fixed last node.
# Long edges: (0, 9) joins two runs, (6, 2) is reversed with its i end fixed, (3, 11) has its j end, the last node, fixed.
SHAPES_B = dict(
    n=12, fixed=(5, 6, 11), gaps=(2,), reverse=(10,), priors=(1, 1), long=((0, 9), (6, 2), (3, 11)), runs=((0, 3), (3, 5), (7, 11)))
# Every node fixed, so T has no run at all: the chain, a prior, and two long edges that add cost only.
SHAPES_ALL_FIXED = dict(n=5, fixed=(0, 1, 2, 3, 4), gaps=(), reverse=(1,), priors=(2,), long=((0, 3), (4, 1)), runs=())
SHAPES = {"shapes_a": SHAPES_A, "shapes_b": SHAPES_B, "all_fixed": SHAPES_ALL_FIXED}


def shape_graph(name):
    if name not in _graphs:
        s = SHAPES[name]
        edges = _chain(s["n"], s["gaps"], s["reverse"]) + list(s["long"]) + [(-1, k) for k in s["priors"]]
        g = _symmetric(R.make_structured(np.random.default_rng(sum(map(ord, name))), s["n"], edges, fixed=s["fixed"], noise=0.01))
        if name == "all_fixed":      # fixed nodes off their truth, or the cost would be noise alone
            rng = np.random.default_rng(9)
            g = (np.array([P @ R.exp_se3(rng.normal(0, 0.05, 6)) for P in g[0]]),) + g[1:]
        _graphs[name] = g
    return _graphs[name]


def graph(name):
    return seam_graph(name) if name in SEAMS else shape_graph(name)


# ---- D. the rejected step ------------------------------------------------------------------------------------------------------------
def rejected_graph():
    """The first solve at lambda = 1e-4 overshoots: F' / F = 1.43 on the restatement, 43 % from the threshold of acceptance."""
    if "rejected" not in _graphs:
        _graphs["rejected"] = _symmetric(R.make_graph(np.random.default_rng(3), 40, 4, noise=0.01, drift=0.5))
    return _graphs["rejected"]


# The same generator and seed at a tenth and at 0.6 of that drift: the first trial is accepted (F' / F = 0.05 and 0.78 on the
# restatement), so optimize(max_iters = 1) returns P Exp(delta).  At 0.05 the first step has |phi|^2 on both sides of 1e-2 (four
# nodes below, 35 above, up to 0.6 rad), at 0.3 rotations up to 2 rad.
ACCEPTED_DRIFTS = (0.05, 0.3)


def accepted_graph(drift):
    if ("accepted", drift) not in _graphs:
        _graphs[("accepted", drift)] = _symmetric(R.make_graph(np.random.default_rng(3), 40, 4, noise=0.01, drift=drift))
    return _graphs[("accepted", drift)]


# ---- E. the pivot failure that can be reached ---------------------------------------------------------------------------------------
WEAK_PRIOR = 1e-20


def weak_prior_graph():
    """A free 12-node chain whose one anchor, the prior on its last node, weighs 1e-20: at lambda = 0 the last pivot of the chain
    factor is about 1e-20 against 1e-12 x a diagonal entry of 100 and more; any damping makes T definite again."""
    if "weak" not in _graphs:
        g = _symmetric(R.make_graph(np.random.default_rng(4), 12, 0, noise=0.01, fixed=(), n_priors=1))
        assert tuple(g[2][-1]) == (-1, 11)
        g[4][-1] = WEAK_PRIOR * np.eye(6)
        _graphs["weak"] = g
    return _graphs["weak"]
