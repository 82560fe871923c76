"""`python -m libviso_amd.posegraph POSES.txt EDGES.txt OUT.txt` on a 20-node graph: the pose file it writes holds the poses that
PoseGraph.optimize returns for the graph the files describe, exactly (every number of the formats reads back to the same double)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from libviso_amd import PoseGraph, fuse_map, posegraph

import posegraph_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_command_line_writes_the_optimised_poses(viso, tmp_path):
    rng = np.random.default_rng(20)
    p0, fx, ij, Z, info, _ = R.make_graph(rng, 20, 2, noise=0.01, fixed=(0,))
    info = 0.5 * (info + info.transpose(0, 2, 1))
    files = [str(tmp_path / n) for n in ("poses.txt", "edges.txt", "out.txt")]
    fuse_map.write_poses(files[0], p0)
    posegraph.write_edges(files[1], ij, Z, info)
    r = subprocess.run([sys.executable, "-m", "libviso_amd.posegraph"] + files + ["--fix", "0"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "status 1" in r.stdout, r.stdout + r.stderr
    g = PoseGraph(fuse_map.read_poses(files[0]))
    for (i, j), Zk, Ok in zip(*posegraph.read_edges(files[1])):
        g.add_edge(i, j, Zk, Ok)
    g.fix(0)
    want, rep = g.optimize()
    assert rep["status"] == 1 and rep["n_long"] == 2
    got = fuse_map.read_poses(files[2])
    assert got.tobytes() == want.tobytes()
    # and the files hold the graph they were written from, to the last bit
    assert np.array_equal(g.poses[:, :3], p0[:, :3]) and np.array_equal(np.array(g.info), info)
