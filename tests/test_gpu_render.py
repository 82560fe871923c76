"""The ray casting of the TSDF map on the device (include/viso_hip.h, viso_tsdf_render; tsdf_render_kernel in
libviso_amd/csrc/tsdf.hip) against its numpy restatement (tests/render_ref.py), byte for byte on the disparity maps and the weights.

The restatement is fed the entries of tests/tsdf_ref.py, not what the device read back; that the device's entries equal them is
asserted beside it.

Input condition, asserted first on the restatement: fusing reports n_out_of_range == 0 and n_dropped == 0, and in every rendered
view at least half of the pixels are valid and at least one is invalid, so that no test passes by both sides returning nothing.
(A view of one pixel cannot be both: its pixel is valid.)  The scenes are the wall, the slanted plane and the depth step of
tests/render_ref.py with the columns at the right left invalid; at voxel 5.0 the baseline is five times as long, so that the
scene spans several voxels (at 9.7 m the whole view lies inside one voxel of 5 m and every ray sees the wall)."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import TSDF_ENTRY_DTYPE, Param

import render_ref as RR
import tsdf_ref as R
from test_gpu_tsdf import POSE

pytestmark = pytest.mark.gpu

INV = R.INVALID
LOG2 = 21
# voxel, the baseline's factor, max_depth (N = 680, 200, 40 samples), the part of the columns that is invalid
CONFIGS = ((0.05, 1.0, 17.0, 0.1), (0.2, 1.0, 20.0, 0.1), (5.0, 5.0, 100.0, 0.4))


def _param(base_factor=1.0, **kw):
    return Param.default(**dict(dict(base=0.5371 * base_factor, f=721.5377, cu=609.5593, cv=172.854), **kw))


def _condition(d, tag):
    valid = float((d != INV).mean())
    assert valid >= 0.5 and (valid < 1.0 or d.size == 1), (tag, valid)


def _want(entries, voxel, prm, shape, pose, max_depth, min_weight, tag):
    d, w = RR.render(entries, voxel, prm, shape, pose, max_depth, min_weight)
    _condition(d, tag)
    assert ((d == INV) == (w == 0)).all()
    return d, w


def _equal(got, want, tag):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, tag
        assert g.tobytes() == w.tobytes(), (tag, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())


def _fuse(tsdf, frames, prm, voxel, trunc):
    want, st = R.fuse(frames, prm, voxel, trunc, 16, LOG2)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0
    tsdf.clear()
    for m, pose in frames:
        tsdf.fuse(m, prm, pose=pose)
    assert tsdf.entries().tobytes() == want.tobytes() and tsdf.stats() == st
    return want


@pytest.mark.parametrize("shape", [(37, 333), (1, 1), (3, 130)])
@pytest.mark.parametrize("trunc", [1, 3])
def test_device_equals_restatement(viso, shape, trunc):
    """(3, 130): runs that cross the wave boundary at columns 63/64 and 127/128, and a short last wave.  voxel 0.05: no two lanes
    share a voxel; 0.2: mixed; 5.0: a whole wave is one run.  Without a pose and with POSE, each seen from the fusing pose and from a
    second one (moved sideways and turned a little); the scene changes from one combination to the next."""
    n = 0
    for voxel, base_factor, max_depth, hole in CONFIGS:
        # every principal point lies outside the image; the one pixel of (1, 1) looks along the axis, so that its ray stays in the
        # column of voxels that its own measurement filled
        prm = _param(base_factor) if shape[1] > 1 else _param(base_factor, cu=0.25, cv=-0.25)
        assert RR.n_samples(voxel, max_depth) <= 700
        tsdf = libviso_amd.TsdfMap(None, voxel=voxel, trunc_voxels=trunc, capacity_log2=LOG2)
        for fuse_pose in (None, POSE):
            for second in (False, True):
                name = RR.SCENES[n % 3]
                n += 1
                tag = (shape, trunc, voxel, fuse_pose is not None, second, name)
                m = RR.scene_map(name, shape, hole if shape[1] > 1 else 0.0)
                entries = _fuse(tsdf, [(m, fuse_pose)], prm, voxel, trunc)
                view = (RR.sideways(fuse_pose, 0.1 * base_factor, 0.01) if shape[1] > 1 else RR.sideways(fuse_pose, 0.001)) if second else fuse_pose
                want = _want(entries, voxel, prm, shape, view, max_depth, 1, tag)
                if view is None:
                    got = tsdf.render(prm, shape, None, max_depth=max_depth, min_weight=1, weights=True)
                    _equal(got, want, tag)
                    view = np.eye(4)       # and the identity as a matrix gives the same bytes
                got = tsdf.render(prm, shape, view, max_depth=max_depth, min_weight=1, weights=True)
                _equal(got, want, tag)
                assert tsdf.render(prm, shape, view, max_depth=max_depth, min_weight=1).tobytes() == want[0].tobytes()
        tsdf.close()


def test_min_weight_on_a_map_of_two_frames(viso):
    prm = _param()
    shape = (37, 333)
    frames = [(RR.scene_map("step", shape, 0.1), POSE), (RR.scene_map("step", shape, 0.3), RR.sideways(POSE, 0.03))]
    tsdf = libviso_amd.TsdfMap(None, voxel=0.05, capacity_log2=LOG2)
    entries = _fuse(tsdf, frames, prm, 0.05, 3)
    assert (entries["weight"] == 1).any() and (entries["weight"] > 2).any()
    views = []
    for mw in (1, 2):
        want = _want(entries, 0.05, prm, shape, POSE, 17.0, mw, ("two frames", mw))
        _equal(tsdf.render(prm, shape, POSE, max_depth=17.0, min_weight=mw, weights=True), want, ("two frames", mw))
        assert (want[1][want[0] != INV] >= mw).all()
        views.append(want[0])
    assert views[0].tobytes() != views[1].tobytes()
    # the default is min_weight 2 and max_depth 40
    assert tsdf.render(prm, (3, 130), POSE).tobytes() == RR.render(entries, 0.05, prm, (3, 130), POSE, 40.0, 2)[0].tobytes()
    tsdf.close()


def test_views_of_one_call_and_other_sizes(viso):
    prm = _param()
    shape = (37, 333)
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=LOG2)
    entries = _fuse(tsdf, [(RR.scene_map("plane", shape, 0.1), POSE)], prm, 0.2, 3)
    poses = np.stack([POSE, RR.sideways(POSE, 0.1, 0.01), RR.sideways(POSE, -0.05, -0.005)])
    d, w = tsdf.render(prm, shape, poses, max_depth=20.0, min_weight=1, weights=True)
    assert d.shape == w.shape == (3,) + shape
    for i in range(3):
        one = tsdf.render(prm, shape, poses[i], max_depth=20.0, min_weight=1, weights=True)
        _equal((d[i], w[i]), one, ("views", i))
        _equal(one, _want(entries, 0.2, prm, shape, poses[i], 20.0, 1, ("views", i)), ("views", i))
    assert d[0].tobytes() != d[1].tobytes() != d[2].tobytes()
    # a size other than the fused maps': a window of them, the principal point moved with it
    small = (20, 50)
    prm2 = _param(cu=prm.cu - 150.0, cv=prm.cv - 9.0)
    want = RR.render(entries, 0.2, prm2, small, POSE, 20.0, 1)
    assert want[0].tobytes() == d[0][9:29, 150:200].tobytes() and (want[0] != INV).mean() >= 0.5
    _equal(tsdf.render(prm2, small, POSE, max_depth=20.0, min_weight=1, weights=True), want, "window")
    # a principal point outside the image on the other side, above and to the left (in every other test it is below and to the right)
    prm3 = _param(cu=-400.25, cv=-30.5)
    entries = _fuse(tsdf, [(RR.scene_map("step", small, 0.1), POSE)], prm3, 0.2, 3)
    for view in (POSE, RR.sideways(POSE, 0.05, 0.005)):
        _equal(tsdf.render(prm3, small, view, max_depth=20.0, min_weight=1, weights=True),
               _want(entries, 0.2, prm3, small, view, 20.0, 1, "outside"), "outside")
    tsdf.close()


def test_more_views_than_one_group(viso):
    """The views of a call go to the device in groups of 16384 (VOXEL_GROUP): 16384 + 3 views of 1 x 3 pixels with five poses in
    turn, so that neighbouring views differ and every view of the second group has a pose that is not the first group's at its
    place."""
    prm = _param(cu=1.3, cv=0.4)
    shape = (1, 3)
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=LOG2)
    entries = _fuse(tsdf, [(RR.scene_map("step", (9, 40)), POSE)], _param(cu=20.3, cv=4.4), 0.2, 3)
    five = np.stack([RR.sideways(POSE, 0.04 * i - 0.08, 0.004 * i) for i in range(5)])
    want = [RR.render(entries, 0.2, prm, shape, T, 20.0, 1) for T in five]
    assert sum(int((d != INV).sum()) for d, _ in want) >= 8 and len({d.tobytes() for d, _ in want}) > 1
    n = 16384 + 3
    d, w = tsdf.render(prm, shape, five[np.arange(n) % 5], max_depth=20.0, min_weight=1, weights=True)
    assert d.shape == (n,) + shape
    assert d.tobytes() == np.stack([want[i % 5][0] for i in range(n)]).tobytes()
    assert w.tobytes() == np.stack([want[i % 5][1] for i in range(n)]).tobytes()
    tsdf.close()


def test_render_changes_nothing_and_refusals(viso):
    prm = _param()
    shape = (37, 333)
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=LOG2)
    _fuse(tsdf, [(RR.scene_map("wall", shape, 0.1), POSE)], prm, 0.2, 3)
    before = (tsdf.entries().tobytes(), tsdf.stats(), [x.tobytes() for x in tsdf.mesh()])
    assert (tsdf.render(prm, shape, POSE, max_depth=20.0, min_weight=1) != INV).any()
    assert before == (tsdf.entries().tobytes(), tsdf.stats(), [x.tobytes() for x in tsdf.mesh()])
    # max_depth against the map's own step: N = floor(max_depth / 0.1) in 1 .. 65536
    for max_depth in (0.09, 6553.75):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            tsdf.render(prm, (1, 1), POSE, max_depth=max_depth)
        assert b"viso_tsdf_render" in tsdf.L.viso_last_error()
    assert tsdf.render(prm, (1, 1), POSE, max_depth=0.1).shape == (1, 1)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        tsdf.render(prm, shape, POSE, min_weight=0)
    assert before == (tsdf.entries().tobytes(), tsdf.stats(), [x.tobytes() for x in tsdf.mesh()])
    tsdf.close()
    # an overflowed map refuses; cleared, it renders nothing
    small = libviso_amd.TsdfMap(None, capacity_log2=10)
    many = np.zeros(1500, TSDF_ENTRY_DTYPE)
    many["k"][:, 0] = np.arange(1500) + 500
    many["weight"], many["sum"] = 1, -7
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        small.add_entries(many)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        small.render(prm, (3, 130), POSE)
    small.clear()
    d, w = small.render(prm, (3, 130), POSE, weights=True)
    assert (d == INV).all() and not w.any()
    small.close()
    # a map that outlives its context
    ctx = libviso_amd.Context(0)
    own = libviso_amd.TsdfMap(ctx, capacity_log2=13)
    assert (own.render(prm, (3, 130), POSE) == INV).all()
    ctx.close()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        own.render(prm, (3, 130), POSE)
    own.close()


def test_full_frame_once(viso):
    prm = _param()
    shape = (376, 1241)
    frames = [(RR.scene_map("wall", shape, 0.05), POSE)]
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=23)
    want, st = R.fuse(frames, prm, 0.2, 3, 16, 23)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0
    tsdf.fuse(frames[0][0], prm, pose=POSE)
    view = RR.sideways(POSE, 0.2, 0.01)
    d, w = RR.render(want, 0.2, prm, shape, view, 30.0, 1)
    _condition(d, "full frame")
    got = tsdf.render(prm, shape, view, max_depth=30.0, min_weight=1, weights=True)
    print(f"full frame: {len(want)} voxels, {(d != INV).mean():.3f} of the pixels valid")
    _equal(got, (d, w), "full frame")
    tsdf.close()
