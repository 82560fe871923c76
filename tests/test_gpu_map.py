"""The voxel map on the device (include/viso_hip.h, viso_map_* / viso_batch_fuse_disparities; libviso_amd/csrc/voxelmap.hip)
against its numpy restatement (tests/map_ref.py), bit for bit on the sorted entry arrays, and against the plane the slanted pair was
rendered from.

Input condition of the bit-exact tests: the restatement itself reports n_out_of_range == 0 and n_dropped == 0 (asserted first), so
that no test passes by both sides dropping the same points.  The deliberate range and overflow cases are the exception."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import hostmath, synth
from libviso_amd.abi import MAP_ENTRY_DTYPE, MatchParams, Param

import disparity_ref as DR
import map_ref as M
from test_speckle_cpu import random_map

pytestmark = pytest.mark.gpu

INV = M.INVALID
POSE = np.linalg.inv(hostmath.tr2mat([0.013, -0.021, 0.007, 0.31, -0.12, 1.47]))   # a rotation and a translation
LOG2 = 21                                                                         # 2 M slots: four times the largest frame's pixels


def _param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)   # non-integer cu, cv


def _same(got, want):
    assert got.dtype == MAP_ENTRY_DTYPE == M.ENTRY
    return got.shape == want.shape and np.array_equal(got, want) and got.tobytes() == want.tobytes()


def _clean(st):
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0, st
    return st


def _check_counters(vmap, st):
    got = vmap.stats()
    for k in ("n_points", "n_out_of_range", "n_dropped", "n_occupied"):
        assert got[k] == st[k], (k, got, st)
    assert st["n_occupied"] <= got["n_inserts"] <= st["n_points"] - st["n_out_of_range"] or st["n_points"] == 0


def _chained_poses(nf=5):
    """Poses of a synthetic sequence through hostmath.chain_poses: one 4 x 4 matrix per frame (frames whose solve failed keep the
    identity)."""
    seq = synth.make_sequence(3, nf, n_kp=400, width=500, height=200)
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, nf, 400)
    b.upload(seq["kp"], seq["desc"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=1)
    b.run()
    tr, ok, _ = b.poses()
    b.close(); ctx.close()
    poses, valid = hostmath.chain_poses(tr, ok)
    assert len(valid) >= 2
    return [poses[k + 1] for k in range(len(valid))]


@pytest.mark.parametrize("shape", [(376, 1241), (37, 333), (1, 1)])
def test_device_equals_restatement(viso, shape):
    rng = np.random.default_rng(shape[0] * 3 + shape[1])
    m = random_map(rng, *shape, spread=2100, invalid=0.2)
    m.flat[0] = 0 if m.size > 1 else 400      # a disparity of 0 never divides
    m.flat[-1] = 15 if m.size > 1 else 400
    prm = _param()
    chained = _chained_poses()
    for voxel in (0.05, 0.2, 1.0, 1000.0):
        for md in (1, 16, 160):
            vmap = libviso_amd.VoxelMap(None, voxel=voxel, min_disp16=md, capacity_log2=LOG2)
            for name, pose in (("none", None), ("identity", np.eye(4)), ("rigid", POSE), ("chained", chained[-1])):
                want, st = M.fuse([(m, pose)], prm, voxel, md, LOG2)
                _clean(st)
                vmap.clear()
                vmap.fuse(m, prm, pose=pose)
                got = vmap.entries()
                assert _same(got, want), (shape, voxel, md, name)
                _check_counters(vmap, st)
                assert vmap.count() == len(want) and int(got["count"].sum()) == st["n_points"] == int(((m != INV) & (m >= md)).sum())
                for mc in (2, 5):
                    assert _same(vmap.entries(mc), want[want["count"] >= mc]) and vmap.count(mc) == int((want["count"] >= mc).sum())
                c = vmap.centroids()
                assert np.array_equal(c.view(np.uint32), M.centroids(want, voxel).view(np.uint32))
            vmap.close()


def test_chained_poses_over_several_frames(viso):
    """Several frames, each with its own pose from hostmath.chain_poses, into one map."""
    rng = np.random.default_rng(9)
    prm = _param()
    chained = _chained_poses()
    frames = [(random_map(rng, 60, 333, spread=1800, invalid=0.3), T) for T in chained]
    want, st = M.fuse(frames, prm, 0.2, 16, LOG2)
    _clean(st)
    vmap = libviso_amd.VoxelMap(None, voxel=0.2, capacity_log2=LOG2)
    for m, T in frames:
        vmap.fuse(m, prm, pose=T)
    assert _same(vmap.entries(), want)
    _check_counters(vmap, st)
    vmap.close()


def test_degenerate_inputs(viso):
    prm = _param()
    vmap = libviso_amd.VoxelMap(None, voxel=1000.0, min_disp16=16, capacity_log2=10)
    rows, cols = 376, 1241
    vmap.fuse(np.full((rows, cols), INV, np.int16), prm)
    assert len(vmap.entries()) == 0 and vmap.count() == 0
    assert vmap.stats() == dict(n_points=0, n_inserts=0, n_out_of_range=0, n_dropped=0, n_occupied=0)
    assert vmap.centroids().shape == (0, 3)
    # every pixel in one voxel: the worst contention.  The camera looks along +z from the origin, where eight voxels meet, so the
    # scene (a plane 19 m ahead, 34 m wide) is moved to the middle of voxel (0, 0, 0) first
    m = np.full((rows, cols), 320, np.int16)
    T = np.eye(4); T[:3, 3] = 500.0
    want, st = M.fuse([(m, T)], prm, 1000.0, 16, 10)
    _clean(st)
    assert len(want) == 1 and want["count"][0] == rows * cols and want["k"][0].tolist() == [0, 0, 0]
    vmap.fuse(m, prm, pose=T)
    got = vmap.entries()
    assert _same(got, want) and got["count"][0] == rows * cols
    _check_counters(vmap, st)
    # one insertion per run of equal keys inside a wave: at most one per 64 pixels here, and at least one
    assert 1 <= vmap.stats()["n_inserts"] <= (rows * cols + 63) // 64 + rows
    vmap.close()


def test_out_of_range_points_are_counted_not_inserted(viso):
    """The deliberate range case: a voxel so small that part of the scene lies beyond 2^30 cells."""
    rng = np.random.default_rng(4)
    m = random_map(rng, 37, 333, spread=2100, invalid=0.2)
    prm = _param()
    voxel = 2e-4
    want, st = M.fuse([(m, POSE)], prm, voxel, 1, LOG2)
    assert 0 < st["n_out_of_range"] < st["n_points"] and st["n_dropped"] == 0 and len(want) > 0
    vmap = libviso_amd.VoxelMap(None, voxel=voxel, min_disp16=1, capacity_log2=LOG2)
    vmap.fuse(m, prm, pose=POSE)
    assert _same(vmap.entries(), want)
    _check_counters(vmap, st)
    # a pose that is not finite is refused, and the map stays as it was
    bad = POSE.copy(); bad[3, 3] = np.nan
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        vmap.fuse(m, prm, pose=bad)
    assert _same(vmap.entries(), want)
    vmap.close()


@pytest.mark.parametrize("method", ["bm", "sgm"])
def test_maps_of_both_methods(viso, method):
    L, R, _ = DR.slanted_pair()
    raw = libviso_amd.stereo_disparity(L, R) if method == "bm" else libviso_amd.stereo_sgm(L, R)
    prm = _param()
    vmap = libviso_amd.VoxelMap(None, capacity_log2=LOG2)
    for d16 in (raw, libviso_amd.filter_speckles(raw)):
        for pose in (None, POSE):
            want, st = M.fuse([(d16, pose)], prm, capacity_log2=LOG2)
            _clean(st)
            vmap.clear()
            vmap.fuse(d16, prm, pose=pose)
            assert _same(vmap.entries(), want)
            _check_counters(vmap, st)
            ins = vmap.stats()["n_inserts"]
            print(f"{method}: {st['n_points']} points, {ins} insertions ({ins / st['n_points']:.4f} a point), {len(want)} voxels")
            for mc in (2, 5):
                assert _same(vmap.entries(mc), want[want["count"] >= mc])
    vmap.close()


def _batch_with_maps(ctx, seq, **disp):
    nf, cap = seq["kp"].shape[0], seq["kp"].shape[2]
    b = libviso_amd.Batch(ctx, nf, cap)
    b.upload_images(seq["images"], seq["kp"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=3)
    b.set_disparity(**disp)
    return b


def _frame_poses(b):
    tr, ok, _ = b.poses()
    poses, valid = hostmath.chain_poses(tr, ok)
    full = np.tile(np.eye(4), (b.nf, 1, 1))
    for k, t in enumerate(valid):
        full[t] = poses[k + 1]
    return full, valid


def test_resident_path_partitions_and_on_off(viso):
    seq = synth.make_subpixel_image_sequence(4, 6, n_kp=500, width=640, height=200)
    prm = seq["param"]
    ctx = libviso_amd.Context(0)
    b = _batch_with_maps(ctx, seq, num_disp=64)
    nf = b.nf
    vmap = libviso_amd.VoxelMap(ctx, capacity_log2=LOG2)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.fuse_disparities(vmap, np.tile(np.eye(4), (nf, 1, 1)))      # no run has computed the maps
    b.set_speckle(max_size=50)
    b.run_images()
    T, valid = _frame_poses(b)
    assert len(valid) >= 2
    before = (b.poses(), [b.matches(w, t) for w in range(3) for t in range(nf)], b.disparities())
    maps = [b.disparity(t) for t in range(nf)]
    want, st = M.fuse([(maps[t], T[t]) for t in range(nf)], prm, capacity_log2=LOG2)
    _clean(st)
    # the resident path, all frames in one call
    b.fuse_disparities(vmap, T)
    whole = vmap.entries()
    assert _same(whole, want)
    _check_counters(vmap, st)
    # ... equals fusing the downloaded maps one by one, in reverse order
    one = libviso_amd.VoxelMap(None, capacity_log2=LOG2)
    for t in reversed(range(nf)):
        one.fuse(maps[t], prm, pose=T[t])
    assert _same(one.entries(), whole)
    # partitions: two maps over disjoint frame sets, joined by add_entries
    a, c = libviso_amd.VoxelMap(ctx, capacity_log2=LOG2), libviso_amd.VoxelMap(ctx, capacity_log2=LOG2)
    b.fuse_disparities(a, T[:2], t0=0, t1=2)
    b.fuse_disparities(c, T[2:], t0=2)
    assert _same(a.entries(), M.fuse([(maps[t], T[t]) for t in range(2)], prm, capacity_log2=LOG2)[0])
    part_c = c.entries()
    a.add_entries(part_c)
    assert _same(a.entries(), whole) and _same(M.merge(part_c, M.fuse([(maps[t], T[t]) for t in range(2)], prm, capacity_log2=LOG2)[0]), whole)
    sa = a.stats()
    assert sa["n_points"] == st["n_points"] and sa["n_occupied"] == st["n_occupied"] and sa["n_dropped"] == 0
    # a saved map loaded into an empty one
    c.clear()
    c.add_entries(whole)
    assert _same(c.entries(), whole) and _same(c.entries(2), whole[whole["count"] >= 2])
    # on / off: the batch's own outputs are byte-identical before and after fusing from it
    after = (b.poses(), [b.matches(w, t) for w in range(3) for t in range(nf)], b.disparities())
    for x, y in zip(before[0], after[0]):
        assert np.array_equal(x, y) and x.tobytes() == y.tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(before[1], after[1])) and np.array_equal(before[2], after[2])
    # argument errors of the resident call
    for bad in (dict(t0=-1, t1=1, poses=T[:2]), dict(t0=0, t1=nf + 1, poses=np.tile(np.eye(4), (nf + 1, 1, 1))), dict(t0=2, t1=2, poses=T[:0])):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b.fuse_disparities(vmap, bad["poses"], t0=bad["t0"], t1=bad["t1"])
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.fuse_disparities(one, T)          # a map of another context
    nan = T.copy(); nan[1, 0, 0] = np.inf
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.fuse_disparities(vmap, nan)
    assert _same(vmap.entries(), whole)
    for v in (one, a, c):
        v.close()
    # a map that outlives its context: every call answers with a code, and destroy frees it
    b.close(); ctx.close()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        vmap.stats()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        vmap.entries()
    vmap.close()
    assert vmap.h is None


def test_overflow_is_an_error_code_and_clear_recovers(viso):
    """A table of 2^10 slots fed 2000 cells.  The probe loop visits every slot at most once, so the full table costs the points that
    find no slot 1024 probes each and nothing else."""
    prm = Param.default(base=1.0, f=2.0, cu=0.0, cv=0.0)
    wide = np.full((1, 2000), 16, np.int16)           # d = 1 px: X = x, one voxel of 0.5 m per pixel
    _, st = M.fuse([(wide, None)], prm, 0.5, 1, 10)
    assert st["n_dropped"] > 0 and st["n_occupied"] == 1024
    vmap = libviso_amd.VoxelMap(None, voxel=0.5, min_disp16=1, capacity_log2=10)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        vmap.fuse(wide, prm)
    got = vmap.stats()
    assert got["n_dropped"] == 2000 - 1024 and got["n_occupied"] == 1024 and got["n_points"] == 2000
    small = np.full((1, 100), 16, np.int16)
    for call in (vmap.entries, vmap.count, lambda: vmap.fuse(small, prm), lambda: vmap.add_entries(np.zeros(0, MAP_ENTRY_DTYPE))):
        with pytest.raises(libviso_amd.VisoError, match="-4"):
            call()
    vmap.clear()
    want, st = M.fuse([(small, None)], prm, 0.5, 1, 10)
    _clean(st)
    vmap.fuse(small, prm)
    assert _same(vmap.entries(), want) and len(want) == 100
    _check_counters(vmap, st)
    # add_entries overflows the same way
    many = np.zeros(1500, MAP_ENTRY_DTYPE)
    many["k"][:, 0] = np.arange(1500) + 500
    many["count"] = 1
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        vmap.add_entries(many)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        vmap.entries()
    vmap.clear()
    vmap.add_entries(many[:1024])          # exactly full: no drop
    assert _same(vmap.entries(), M.merge(many[:1024])) and vmap.stats()["n_occupied"] == 1024
    # entries that are not voxels of a map are refused before the device
    for field, value in (("count", 0), ("k", [1 << 20, 0, 0]), ("k", [0, -(1 << 20) - 1, 0]), ("sum", [1024, 0, 0])):
        bad = many[:1].copy()
        bad[field] = value
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            vmap.add_entries(bad)
    vmap.close()


def test_centroids_of_the_slanted_pair_lie_on_its_plane(viso):
    """slanted_pair renders the plane d*(x, y) = a + b x + c y in disparity space, which is the plane n . P = f base in space with
    n = (b f, c f, a + b cu + c cv) (substitute x = cu + f X / Z, y = cv + f Y / Z, d = f base / Z).  Under a pose P' = R P + t it is
    n' . (P' - t) = f base with n' = R n.

    The bound is derived here, from the error of the unfiltered map against d*.  A pixel's point lies on the pixel's ray at depth
    Z = f base / d; the plane meets that ray at Z* = f base / d*, so the point is at most e = |Z - Z*| |((x - cu) / f, (y - cv) / f, 1)|
    from the plane (rigid poses keep distances).  A voxel's centroid is the mean of its points and the distance from a plane is
    convex, so the centroid is at most mean(e over the voxel's pixels) from the plane, were it the exact mean.  It is not: each
    offset is floored to the grid of s = voxel / 1024 (the + 0.5 centres it) and each coordinate is rounded once to float32; half a
    voxel diagonal, voxel sqrt(3) / 2, covers both with room to spare and is the bound's second term.  Which pixels share a voxel comes from
    the restatement, which the device has to equal anyway."""
    L, R, dtrue = DR.slanted_pair()
    raw = libviso_amd.stereo_disparity(L, R)
    prm = _param()
    f, cu, cv, base = prm.f, prm.cu, prm.cv, prm.base
    rows, cols = raw.shape
    # the plane's coefficients from the rendered truth (exactly linear)
    a = dtrue[0, 0]; b = (dtrue[0, -1] - dtrue[0, 0]) / (cols - 1); c = (dtrue[-1, 0] - dtrue[0, 0]) / (rows - 1)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    assert np.allclose(dtrue, a + b * xx + c * yy, rtol=0, atol=1e-9)
    n = np.array([b * f, c * f, a + b * cu + c * cv])
    voxel, md = 0.2, 16
    for pose in (None, POSE):
        want, st = M.fuse([(raw, pose)], prm, voxel, md, LOG2)
        _clean(st)
        vmap = libviso_amd.VoxelMap(None, voxel=voxel, min_disp16=md, capacity_log2=LOG2)
        vmap.fuse(raw, prm, pose=pose)
        assert _same(vmap.entries(), want)
        cen = vmap.centroids().astype(np.float64)
        vmap.close()
        # per pixel: its error bound e, and the voxel it went to
        use = (raw != INV) & (raw >= md)
        d = raw[use] / 16.0
        Z, Zs = f * base / d, f * base / dtrue[use]
        ray = np.sqrt(((xx[use] - cu) / f) ** 2 + ((yy[use] - cv) / f) ** 2 + 1.0)
        e = np.abs(Z - Zs) * ray
        g, n_points, n_oor = M.cells(raw, prm, pose, voxel, md)
        assert n_oor == 0 and len(g) == len(e) == n_points
        keys, inv = np.unique(M.keys_of(g >> 10), return_inverse=True)
        assert np.array_equal(keys, M.keys_of(want["k"]))
        e_sum = np.zeros(len(keys)); np.add.at(e_sum, inv, e)
        bound = e_sum / want["count"] + voxel * np.sqrt(3.0) / 2.0
        if pose is None:
            dist = np.abs(cen @ n - f * base) / np.linalg.norm(n)
        else:
            dist = np.abs((cen - pose[:3, 3]) @ (pose[:3, :3] @ n) - f * base) / np.linalg.norm(n)
        print(f"pose {'none' if pose is None else 'rigid'}: {len(keys)} voxels, centroid distance from the plane: median {np.median(dist):.4f} m, "
              f"max {dist.max():.4f} m; bound: median {np.median(bound):.4f} m, smallest margin {(bound - dist).min():.4f} m")
        assert (dist <= bound).all()
