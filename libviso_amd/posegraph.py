"""Pose-graph optimisation on the device (include/viso_hip.h, "pose graph"; csrc/posegraph.hip): a graph of poses, relative-pose
edges and priors, its linearisation and its Levenberg-Marquardt optimum; the edges of a batch's odometry and the prior of an
alignment; and a command line from a pose file and an edge file to the pose file `fuse_map --repose` takes:

    python -m libviso_amd.posegraph POSES.txt EDGES.txt OUT.txt [--fix K ...] [--max-iters N] [--eps-step E]

POSES.txt is a KITTI pose file (12 numbers a line).  A line of EDGES.txt is `i j`, the 12 numbers of Z's first three rows and the 21
entries of the upper triangle of the information matrix, row by row; i = -1 is a prior."""
import argparse
import ctypes as C
import sys

import numpy as np

from . import VisoError, _call, _ctx_h, _f64, _i32, load
from .abi import MOTION_COV_DTYPE, POSE_GRAPH_REPORT, TSDF_ALIGNMENT_DTYPE, ptr

_IU = np.triu_indices(6)


def _pose44(where, T):
    T = np.asarray(T, np.float64)
    if T.shape == (3, 4):
        T = np.vstack([T, [0.0, 0.0, 0.0, 1.0]])
    if T.shape != (4, 4):
        raise ValueError(f"{where}: a pose is a 4 x 4 (or 3 x 4) matrix")
    return T


class PoseGraph:
    """Poses [n][4][4] (camera to world), edges (i, j, Z, info) with Z measuring P_i^-1 P_j and info the 6 x 6 information of the
    error in the tangent order (phi, rho), priors (i = -1: Z measures P_j), and the nodes that stay as given."""

    def __init__(self, poses):
        self.poses = _f64(poses).reshape(-1, 4, 4).copy()
        self.fixed = np.zeros(len(self.poses), np.int32)
        self.ij, self.Z, self.info = [], [], []

    def add_edge(self, i, j, Z, info):
        info = np.asarray(info, np.float64)
        if info.shape != (6, 6):
            raise ValueError("PoseGraph.add_edge: the information matrix is 6 x 6")
        self.ij.append((int(i), int(j)))
        self.Z.append(_pose44("PoseGraph.add_edge", Z))
        self.info.append(info)

    def add_prior(self, j, pose, info):
        self.add_edge(-1, j, pose, info)

    def fix(self, k):
        self.fixed[int(k)] = 1

    def arrays(self):
        """(poses, fixed, ij [m][2] int32, Z [m][4][4], info [m][6][6]) as contiguous arrays: what the C calls take."""
        return (_f64(self.poses), _i32(self.fixed), _i32(np.reshape(self.ij, (-1, 2))), _f64(np.reshape(self.Z, (-1, 4, 4))),
                _f64(np.reshape(self.info, (-1, 6, 6))))

    def _graph_args(self, ctx):
        poses, fixed, ij, Z, info = self._held = self.arrays()
        return (_ctx_h(ctx), len(poses), ptr(poses, C.c_double), ptr(fixed, C.c_int32), len(ij), ptr(ij, C.c_int32), ptr(Z, C.c_double),
                ptr(info, C.c_double))

    def linearize(self, lam=0.0, ctx=None):
        """viso_pose_graph_linearize: (cost, grad [n][6], step [n][6]) at the graph's poses, the step of one solve at lambda = lam."""
        n = len(self.poses)
        cost, grad, step = C.c_double(0.0), np.zeros((n, 6)), np.zeros((n, 6))
        _call(load().viso_pose_graph_linearize, *self._graph_args(ctx), float(lam), C.byref(cost), ptr(grad, C.c_double), ptr(step, C.c_double))
        return cost.value, grad, step

    def optimize(self, max_iters=50, eps_step=1e-10, ctx=None, trace=False):
        """viso_pose_graph_optimize: (poses [n][4][4], report dict) and, with trace, the solves' entries [iters][5] (F, F', lambda,
        max |delta|, accepted).  A negative status raises VisoError, with the report as its .report."""
        n = len(self.poses)
        out, rep = np.zeros((n, 4, 4)), np.zeros(8)
        tr = np.zeros((int(max_iters) if trace else 0, 5))
        _call(load().viso_pose_graph_optimize, *self._graph_args(ctx), int(max_iters), float(eps_step), ptr(out, C.c_double), ptr(rep, C.c_double),
              ptr(tr, C.c_double) if trace else None, len(tr))
        report = {k: (float(v) if k in ("cost_initial", "cost_final", "lambda", "last_step") else int(v)) for k, v in zip(POSE_GRAPH_REPORT, rep)}
        if report["status"] < 0:
            err = VisoError(f"PoseGraph.optimize: status {report['status']} after {report['iters']} solves "
                            + ("(a factorisation's pivot failed)" if report["status"] == -2 else "(a number is not finite)"))
            err.report = report
            raise err
        return (out, report, tr[:report["iters"]].copy()) if trace else (out, report)


def motion_edge(tr, cov):
    """viso_motion_edge (host only): (Z [4][4], info [6][6]) of one solved frame's motion tr with covariance cov [6][6]."""
    tr, cov = _f64(np.reshape(tr, 6)), _f64(np.reshape(cov, (6, 6)))
    Z, info = np.zeros((4, 4)), np.zeros((6, 6))
    _call(load().viso_motion_edge, ptr(tr, C.c_double), ptr(cov, C.c_double), ptr(Z, C.c_double), ptr(info, C.c_double))
    return Z, info


def motion_edges(tr, ok, cov):
    """The odometry edges of a batch's outputs (Batch.poses' tr and ok, Batch.covariances' records) between the poses of
    hostmath.chain_poses' list: (edges [(i, j, Z, info)], skipped frames).  A frame with ok == 0 pushed no pose; a frame whose
    covariance has status != 1 has no edge.  Both are listed in `skipped` and not bridged: that is the caller's decision."""
    tr, ok = _f64(np.reshape(tr, (-1, 6))), _i32(ok)
    cov = np.ascontiguousarray(cov, MOTION_COV_DTYPE)
    if len(ok) != len(tr) or len(cov) != len(tr):
        raise ValueError("motion_edges: tr, ok and cov need one entry per frame")
    edges, skipped, k = [], [], 0
    for t in range(len(tr)):
        if not ok[t]:
            skipped.append(t)
            continue
        k += 1
        if cov[t]["status"] != 1:
            skipped.append(t)
            continue
        edges.append((k - 1, k) + motion_edge(tr[t], cov[t]["cov"]))
    return edges, skipped


def alignment_prior(record):
    """(pose [4][4], info [6][6]) of a TSDF_ALIGNMENT_DTYPE record: its covariance is in the order (v, omega), the prior's
    information in (phi, rho)."""
    rec = np.asarray(record, TSDF_ALIGNMENT_DTYPE).reshape(())
    perm = [3, 4, 5, 0, 1, 2]
    cov = np.asarray(rec["cov"], np.float64)[np.ix_(perm, perm)]
    return np.array(rec["pose"], np.float64), np.linalg.inv(0.5 * (cov + cov.T))


# ---- files -------------------------------------------------------------------------------------------------------------------------
def write_edges(path, ij, Z, info):
    """An edge file: `i j`, Z's first three rows, the upper triangle of the information matrix; every number reads back exactly."""
    with open(path, "w") as f:
        for (i, j), Zk, Ok in zip(np.reshape(ij, (-1, 2)), np.reshape(Z, (-1, 4, 4)), np.reshape(info, (-1, 6, 6))):
            f.write("%d %d " % (i, j) + " ".join("%.17g" % v for v in list(Zk[:3].reshape(-1)) + list(Ok[_IU])) + "\n")


def read_edges(path):
    """(ij [m][2] int32, Z [m][4][4], info [m][6][6]) of an edge file."""
    ij, Z, info = [], [], []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            t = line.split()
            if not t:
                continue
            if len(t) != 35:
                raise ValueError(f"{path}:{ln}: expected 2 + 12 + 21 numbers, found {len(t)}")
            ij.append((int(t[0]), int(t[1])))
            v = np.array([float(x) for x in t[2:]])
            Zk, Ok = np.eye(4), np.zeros((6, 6))
            Zk[:3] = v[:12].reshape(3, 4)
            Ok[_IU] = v[12:]
            Z.append(Zk)
            info.append(Ok + np.triu(Ok, 1).T)
    return np.array(ij, np.int32).reshape(-1, 2), np.array(Z).reshape(-1, 4, 4), np.array(info).reshape(-1, 6, 6)


def main(argv=None):
    from .fuse_map import read_poses, write_poses
    ap = argparse.ArgumentParser(prog="python -m libviso_amd.posegraph", description=__doc__.split("\n\n")[0])
    ap.add_argument("poses")
    ap.add_argument("edges")
    ap.add_argument("out")
    ap.add_argument("--fix", type=int, action="append", default=[], metavar="K", help="a node that stays as given (repeatable)")
    ap.add_argument("--max-iters", type=int, default=50)
    ap.add_argument("--eps-step", type=float, default=1e-10)
    a = ap.parse_args(argv)
    g = PoseGraph(read_poses(a.poses))
    for (i, j), Z, info in zip(*read_edges(a.edges)):
        g.add_edge(i, j, Z, info)
    for k in a.fix:
        g.fix(k)
    poses, rep = g.optimize(max_iters=a.max_iters, eps_step=a.eps_step)
    write_poses(a.out, poses)
    print("posegraph: status %d after %d solves, cost %.9g -> %.9g, %d long edges, %d rejected" %
          (rep["status"], rep["iters"], rep["cost_initial"], rep["cost_final"], rep["n_long"], rep["n_rejected"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
