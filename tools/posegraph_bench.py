"""The pose-graph optimiser (include/viso_hip.h, "pose graph") on a synthetic loop trajectory of 4541 poses (the
length of KITTI sequence 00), seeded, with the tests' measurement noise, at L = 1, 16, 64, 256 long edges: wall time of one
`optimize` and of one `linearize` with its step (medians of 7 with min-max; the host clock goes around calls that end in a
synchronise), and beside them the yardstick on the host, the restatement's normal equations solved by scipy's sparse direct solver.

    python tools/posegraph_bench.py [--poses N] [--long L ...] [--repeat R] [--no-host]
    python tools/posegraph_bench.py --kernel-only --long 64      # the run to put under rocprofv3 --kernel-trace --stats

One JSON line a row.  The restatement (tests/posegraph_ref.py) makes the graph and the yardstick; it is test code, read from here."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import libviso_amd  # noqa: E402
import posegraph_ref as R  # noqa: E402


def make(n, L, seed):
    rng = np.random.default_rng(seed)
    p0, fx, ij, Z, info, truth = R.make_graph(rng, n, L, noise=0.01, drift=0.002)
    info = 0.5 * (info + info.transpose(0, 2, 1))
    g = libviso_amd.PoseGraph(p0)
    for (i, j), Zk, Ok in zip(ij, Z, info):
        g.add_edge(i, j, Zk, Ok)
    g.fix(0)
    return g, (p0, fx, ij, Z, info), truth


def timed(fn, repeat):
    fn()   # warm: the first call of a process loads the code object
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(t)), min_ms=min(t), max_ms=max(t)), out


def host_step(arrays, lam):
    """The restatement's normal equations over the free nodes as a sparse matrix, and the step by scipy's spsolve: (assemble ms, solve ms, delta)."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import spsolve
    p0, fx, ij, Z, info = arrays
    n = len(p0)
    t0 = time.perf_counter()
    rows, cols, vals, g = [], [], [], np.zeros((n, 6))
    for e in range(len(ij)):
        i, j = int(ij[e][0]), int(ij[e][1])
        r, Ji, Jj = R.edge_terms(p0, i, j, Z[e])
        ends = [(a, J) for a, J in ((i, Ji), (j, Jj)) if a >= 0 and not fx[a]]
        for a, Ja in ends:
            g[a] += Ja.T @ info[e] @ r
            for b, Jb in ends:
                blk = Ja.T @ info[e] @ Jb
                rr, cc = np.meshgrid(np.arange(6 * a, 6 * a + 6), np.arange(6 * b, 6 * b + 6), indexing="ij")
                rows.append(rr.ravel()); cols.append(cc.ravel()); vals.append(blk.ravel())
    H = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * n, 6 * n))
    free = np.flatnonzero(np.repeat(np.asarray(fx) == 0, 6))
    Hf = H[free][:, free].tocsc()
    Hf = Hf + lam * sp.diags(Hf.diagonal())
    t1 = time.perf_counter()
    d = np.zeros(6 * n)
    d[free] = spsolve(Hf.tocsc(), -g.reshape(-1)[free])
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, d.reshape(n, 6)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--poses", type=int, default=4541)
    ap.add_argument("--long", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--seed", type=int, default=4541)
    ap.add_argument("--no-host", action="store_true", help="leave the scipy yardstick out")
    ap.add_argument("--kernel-only", action="store_true", help="one optimize and one linearize per L and nothing else")
    a = ap.parse_args(argv)
    for L in a.long:
        g, arrays, truth = make(a.poses, L, a.seed)
        if a.kernel_only:
            g.optimize()
            g.linearize(lam=1e-4)
            continue
        t_opt, (poses, rep) = timed(lambda: g.optimize(), a.repeat)
        t_lin, (cost, grad, step) = timed(lambda: g.linearize(lam=1e-4), a.repeat)
        row = dict(leg="pose_graph", n_poses=a.poses, n_edges=len(arrays[2]), n_long=L, columns=6 * L + 1, optimize=t_opt, linearize_with_step=t_lin,
                   report=rep, optimize_ms_per_solve=t_opt["median_ms"] / max(rep["iters"], 1))
        if not a.no_host:
            try:
                asm_ms, solve_ms, d = host_step(arrays, 1e-4)
                row["host"] = dict(assemble_ms=asm_ms, spsolve_ms=solve_ms, step_rel_diff=float(np.abs(d - step).max() / np.abs(d).max()))
            except ImportError as e:   # no scipy: the yardstick is left out, and says so
                row["host"] = dict(skipped=str(e))
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
