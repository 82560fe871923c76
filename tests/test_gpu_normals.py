"""The surface normals of the TSDF map on the device (include/viso_hip.h, viso_tsdf_vertex_normals and viso_tsdf_render_normals;
tsdf_normal_sample_kernel and tsdf_normal_render_kernel in libviso_amd/csrc/tsdf.hip) against their numpy restatement
(tests/normal_ref.py), byte for byte on the normals, the disparity maps and the weights.

The restatement is fed the entries of tests/tsdf_ref.py, not what the device read back; that the device's entries equal them is
asserted beside it.  The input conditions of tests/test_gpu_render.py are asserted first on the restatement (nothing out of range
or dropped, at least half of a view's pixels valid and at least one invalid), and that normals come out at all.  The maps are fused
from 37 x 333 scenes whatever the view's size: a map fused from three rows is one voxel thick and has no gradient, so the small
views are windows of the fused maps (normal_ref.window)."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import TSDF_ENTRY_DTYPE, TSDF_MESH_VERTEX_DTYPE

import mesh_ref as MR
import normal_ref as N
import render_ref as RR
import tsdf_ref as R
import tsdf_tables as TT
from test_gpu_render import CONFIGS, LOG2, _condition, _fuse, _param
from test_gpu_tsdf import POSE
from test_normals_cpu import branch_trace

pytestmark = pytest.mark.gpu

INV = R.INVALID
FULL = (37, 333)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _equal(got, want, tag):
    assert len(got) == len(want), tag
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, tag
        assert g.tobytes() == w.tobytes(), (tag, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())


def _want(entries, voxel, prm, shape, pose, max_depth, min_weight, tag):
    d, w, n = N.render(entries, voxel, prm, shape, pose, max_depth, min_weight)
    _condition(d, tag)
    assert ((d == INV) == (w == 0)).all() and not n[d == INV].any()
    return d, w, n


@pytest.mark.parametrize("shape", [(37, 333), (1, 1), (3, 130)])
@pytest.mark.parametrize("trunc", [1, 3])
def test_device_equals_restatement(viso, shape, trunc):
    """The grid of test_gpu_render: (3, 130) has runs that cross the wave boundary and a short last wave; voxel 0.05: no two lanes
    share a voxel, 0.2: mixed, 5.0: a whole wave is one run (and a view inside one layer of voxels, where few pixels have a normal).
    Without a pose and with POSE, each seen from the fusing pose and from a second one; the scene changes from one combination to
    the next."""
    n, n_normals = 0, {}
    for voxel, base_factor, max_depth, hole in CONFIGS:
        prm = _param(base_factor)
        win = N.window(prm, shape, FULL, hole, inside=45 if voxel == 5.0 else 20)   # a voxel of 5 m bleeds over 40 columns of the hole
        assert RR.n_samples(voxel, max_depth) <= 700
        tsdf = libviso_amd.TsdfMap(None, voxel=voxel, trunc_voxels=trunc, capacity_log2=LOG2)
        for fuse_pose in (None, POSE):
            for second in (False, True):
                name = RR.SCENES[n % 3]
                n += 1
                tag = (shape, trunc, voxel, fuse_pose is not None, second, name)
                entries = _fuse(tsdf, [(RR.scene_map(name, FULL, hole), fuse_pose)], prm, voxel, trunc)
                view = (RR.sideways(fuse_pose, 0.1 * base_factor, 0.01) if shape[1] > 1 else RR.sideways(fuse_pose, 0.001)) if second else fuse_pose
                want = _want(entries, voxel, win, shape, view, max_depth, 1, tag)
                n_normals[voxel] = n_normals.get(voxel, 0) + int(want[2].any(axis=-1).sum())
                if view is None:
                    _equal(tsdf.normals.render(win, shape, None, max_depth=max_depth, min_weight=1, weights=True), want, tag)
                    view = np.eye(4)       # and the identity as a matrix gives the same bytes
                _equal(tsdf.normals.render(win, shape, view, max_depth=max_depth, min_weight=1, weights=True), want, tag)
                _equal(tsdf.normals.render(win, shape, view, max_depth=max_depth, min_weight=1), (want[0], want[2]), tag)
        tsdf.close()
    print(f"{shape}, T = {trunc}: pixels with a normal by voxel {n_normals}")
    assert n_normals[0.05] >= 2 and n_normals[0.2] >= 2 and (shape[1] == 1 or n_normals[0.2] >= shape[0] * shape[1])


def _gray_image(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def test_same_table_same_outputs(viso):
    """normals.render gives render()'s map and weights on the same table, on a plain and on a gray map, and the gray map's
    normals are the plain map's; gray and normals together are the two calls' outputs."""
    prm = _param()
    frames = [(RR.scene_map("step", FULL, 0.1), POSE), (RR.scene_map("plane", FULL, 0.2), RR.sideways(POSE, 0.03))]
    plain = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=LOG2)
    gray = libviso_amd.TsdfMap(None, gray=True, voxel=0.2, capacity_log2=LOG2)
    for i, (m, pose) in enumerate(frames):
        plain.fuse(m, prm, pose=pose)
        gray.fuse(m, prm, pose=pose, image=_gray_image(FULL, i))
    assert _same(plain.entries(), gray.entries())
    views = np.stack([POSE, RR.sideways(POSE, 0.1, 0.01)])
    for mw in (1, 2):
        base = plain.render(prm, FULL, views, max_depth=20.0, min_weight=mw, weights=True)
        got = plain.normals.render(prm, FULL, views, max_depth=20.0, min_weight=mw, weights=True)
        _equal(got[:2], base, ("plain", mw))
        assert got[2].shape == (2,) + FULL + (3,) and got[2].any(axis=-1).sum() > 5000 and not got[2][got[0] == INV].any()
        d, w, g, n = gray.normals.render(prm, FULL, views, max_depth=20.0, min_weight=mw, weights=True, gray=True)
        _equal((d, w, n), got, ("gray", mw))
        _equal((d, w, g), gray.render(prm, FULL, views, max_depth=20.0, min_weight=mw, weights=True, gray=True), ("gray", mw))
        assert _same(gray.render(prm, FULL, views, max_depth=20.0, min_weight=mw), base[0])
    # the vertices' normals read weight and sum only
    v, tri, g, nv = gray.normals.mesh(1, gray=True)
    pv, ptri, pn = plain.normals.mesh(1)
    assert _same(v, pv) and _same(tri, ptri) and _same(nv, pn) and len(g) == len(v) and nv.any(axis=1).sum() > 100
    plain.close(); gray.close()


def test_vertex_normals_of_a_fused_map(viso):
    prm = _param()
    frames = [(RR.scene_map("step", FULL, 0.1), POSE), (RR.scene_map("plane", FULL, 0.2), RR.sideways(POSE, 0.03))]
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=LOG2)
    entries = _fuse(tsdf, frames, prm, 0.2, 3)
    assert (entries["weight"] == 1).any() and (entries["weight"] >= 2).any()
    for mw in (1, 2):
        v, tri, n = tsdf.normals.mesh(mw)
        want, wm = N.vertex_normals(entries, v, mw)
        got, missing = tsdf.normals.vertices(v, mw, missing=True)
        assert _same(n, want) and _same(got, want) and missing == wm, (mw, missing, wm)
        assert len(v) > 300 and n.any(axis=1).sum() > len(v) // 2
        c = tsdf.surface(mw)
        want_c, wm = N.vertex_normals(entries, N.crossing_vertices(c), mw)
        got_c, missing = tsdf.normals.vertices(c, mw, missing=True)
        assert _same(got_c, want_c) and missing == wm and _same(tsdf.normals.surface(mw), want_c) and len(c) > 200, mw
        # a crossing is the mesh's vertex of dir 1 << axis
        both = {(tuple(x["k"].tolist()), int(x["dir"])): y.tobytes() for x, y in zip(v, n)}
        hits = [both.get((tuple(x["k"].tolist()), 1 << int(x["axis"]))) for x in c]
        assert all(h is None or h == y.tobytes() for h, y in zip(hits, got_c)) and sum(h is not None for h in hits) > 100
    tsdf.close()


def test_vertex_normals_on_hand_built_tables(viso):
    """The random blocks at the origin and at both ends of the key range, where a neighbour's index would leave it, at min_weight
    1, 2, 3; the table of the normal of length zero; and a block of 700 voxels in a table of 2^10 slots, whose probes walk long
    chains.  Every branch of the rule is met, asserted before the device is called."""
    trace, cases = branch_trace()
    assert all(trace[b] > 0 for b in N.BRANCHES), dict(trace)
    chains = TT.chains_block()
    cases.append((("chains",), chains, N.crossing_vertices(R.crossings(chains)), 1))
    cases.append((("chains", "mesh"), chains, MR.mesh(chains, 0.2, 1)[0], 1))
    table, loaded = None, None
    n_absent = 0
    for tag, e, v, mw in cases:
        if loaded is not e:
            if table is not None:
                table.close()
            table, loaded = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=10 if tag[0] == "chains" else 13), e
            table.add_entries(e)
            assert _same(table.entries(), np.asarray(e, TSDF_ENTRY_DTYPE))
        want, wm = N.vertex_normals(e, v, mw)
        got, missing = table.normals.vertices(v, mw, missing=True)
        assert _same(got, want) and missing == wm, (tag, missing, wm)
        assert _same(table.normals.vertices(v, mw), want)
        if len(tag) == 3 and tag[2] == 2:                          # the edges whose ends are absent: (0, 0, 0), and counted
            assert wm > len(v) // 2 and (~want.any(axis=1)).sum() == wm
            n_absent += wm
    assert n_absent > 1000
    # the wave count at its edge: no vertex, and 256 k + 1 of them
    e, v, mw = cases[0][1], cases[0][2], cases[0][3]
    table.close()
    table = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=13)
    table.add_entries(e)
    many = np.concatenate([v] * (1 + 600 // len(v)))
    for n in (0, 1, 257, 513):
        want, wm = N.vertex_normals(e, many[:n], mw)
        got, missing = table.normals.vertices(many[:n], mw, missing=True)
        assert got.shape == (n, 3) and _same(got, want) and missing == wm, n
    # an absent edge at the last voxels that have a neighbour: accepted, missing
    edge = np.zeros(2, TSDF_MESH_VERTEX_DTYPE)
    edge["k"], edge["dir"] = [[R.BIAS - 1, R.BIAS - 2, -R.BIAS], [R.BIAS - 2, R.BIAS - 2, R.BIAS - 2]], [2, 7]
    got, missing = table.normals.vertices(edge, missing=True)
    assert not got.any() and missing == 2
    # the refusals of the range
    for k, d in (((0, 0, 0), 0), ((0, 0, 0), 8), ((R.BIAS - 1, 0, 0), 1), ((0, 0, R.BIAS - 1), 4), ((-R.BIAS - 1, 0, 0), 2), ((0, R.BIAS, 0), 1)):
        bad = many[:3].copy()
        bad["k"][1], bad["dir"][1] = k, d
        assert not N.vertex_ok(bad).all()
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            table.normals.vertices(bad)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        table.normals.vertices(many[:3], min_weight=0)
    table.close()


@pytest.mark.parametrize("name", list(TT.BLOCKS))
def test_render_normals_on_random_blocks(viso, name):
    """Every lane of a wave at a different place in the rule: the sweeps of tests/tsdf_tables.py over one table."""
    e = TT.block_entries(name)
    t = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=13)
    t.add_entries(e)
    n_normals = 0
    for pose, mw, case in TT.block_sweep(name):
        _, voxel, prm, shape, T, max_depth, _ = case
        want = N.render(e, voxel, prm, shape, T, max_depth, mw)
        got = t.normals.render(prm, shape, T, max_depth=max_depth, min_weight=mw, weights=True)
        _equal(got, want, (name, pose, mw))
        n_normals += int(want[2].any(axis=-1).sum())
    assert n_normals > 500
    t.close()


def test_views_of_one_call(viso):
    prm = _param()
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=LOG2)
    entries = _fuse(tsdf, [(RR.scene_map("plane", FULL, 0.1), POSE)], prm, 0.2, 3)
    poses = np.stack([POSE, RR.sideways(POSE, 0.1, 0.01), RR.sideways(POSE, -0.05, -0.005)])
    d, w, n = tsdf.normals.render(prm, FULL, poses, max_depth=20.0, min_weight=1, weights=True)
    assert d.shape == w.shape == (3,) + FULL and n.shape == (3,) + FULL + (3,)
    for i in range(3):
        one = tsdf.normals.render(prm, FULL, poses[i], max_depth=20.0, min_weight=1, weights=True)
        _equal((d[i], w[i], n[i]), one, ("views", i))
        _equal(one, _want(entries, 0.2, prm, FULL, poses[i], 20.0, 1, ("views", i)), ("views", i))
    assert n[0].tobytes() != n[1].tobytes() != n[2].tobytes()
    # more views than one group (16384, VOXEL_GROUP): 16384 + 3 views of 1 x 3 pixels with five poses in turn
    shape = (1, 3)
    win = N.window(prm, (1, 1), FULL)
    five = np.stack([RR.sideways(POSE, 0.04 * i - 0.08, 0.004 * i) for i in range(5)])
    want = [N.render(entries, 0.2, win, shape, T, 20.0, 1) for T in five]
    assert sum(int(x[2].any(axis=-1).sum()) for x in want) >= 8 and len({x[2].tobytes() for x in want}) > 1
    count = 16384 + 3
    got = tsdf.normals.render(win, shape, five[np.arange(count) % 5], max_depth=20.0, min_weight=1, weights=True)
    for j in range(3):
        assert got[j].tobytes() == np.stack([want[i % 5][j] for i in range(count)]).tobytes(), j
    tsdf.close()


def test_calls_change_nothing_and_error_states(viso):
    prm = _param()
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=LOG2)
    _fuse(tsdf, [(RR.scene_map("wall", FULL, 0.1), POSE)], prm, 0.2, 3)
    v = tsdf.mesh()[0]
    before = (tsdf.entries().tobytes(), tsdf.stats(), [x.tobytes() for x in tsdf.mesh()])
    assert tsdf.normals.render(prm, FULL, POSE, max_depth=20.0, min_weight=1)[1].any()
    assert tsdf.normals.vertices(v).any() and tsdf.normals.surface().any()
    assert before == (tsdf.entries().tobytes(), tsdf.stats(), [x.tobytes() for x in tsdf.mesh()])
    # max_depth against the map's own step: N = floor(max_depth / 0.1) in 1 .. 65536
    for max_depth in (0.09, 6553.75):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            tsdf.normals.render(prm, (1, 1), POSE, max_depth=max_depth)
        assert b"viso_tsdf_render_normals" in tsdf.L.viso_last_error()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        tsdf.normals.render(prm, FULL, POSE, min_weight=0)
    assert before == (tsdf.entries().tobytes(), tsdf.stats(), [x.tobytes() for x in tsdf.mesh()])
    tsdf.close()
    # an overflowed map refuses both calls; cleared, it has nothing
    small = libviso_amd.TsdfMap(None, capacity_log2=10)
    many = np.zeros(1500, TSDF_ENTRY_DTYPE)
    many["k"][:, 0] = np.arange(1500) + 500
    many["weight"], many["sum"] = 1, -7
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        small.add_entries(many)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        small.normals.render(prm, (3, 130), POSE)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        small.normals.vertices(v[:5])
    small.clear()
    d, n = small.normals.render(prm, (3, 130), POSE)
    assert (d == INV).all() and not n.any()
    n, missing = small.normals.vertices(v[:5], missing=True)
    assert not n.any() and missing == 5
    small.close()
    # a map that outlives its context
    ctx = libviso_amd.Context(0)
    own = libviso_amd.TsdfMap(ctx, capacity_log2=13)
    assert not own.normals.render(prm, (3, 130), POSE)[1].any() and not own.normals.vertices(v[:5]).any()
    ctx.close()
    for call in (lambda: own.normals.render(prm, (3, 130), POSE), lambda: own.normals.vertices(v[:5])):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            call()
    own.close()
