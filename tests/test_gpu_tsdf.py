"""The TSDF map on the device (include/viso_hip.h, viso_tsdf_* / viso_batch_fuse_tsdf; libviso_amd/csrc/tsdf.hip) against its numpy
restatement (tests/tsdf_ref.py), bit for bit on the sorted entry and crossing arrays, and against the wall and the plane the inputs
were rendered from.

Input condition of the bit-exact tests: the restatement itself reports n_out_of_range == 0 and n_dropped == 0 (asserted first), so
that no test passes by both sides dropping the same samples.  The deliberate range and overflow cases are the exception."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import hostmath, synth
from libviso_amd.abi import TSDF_CROSSING_DTYPE, TSDF_ENTRY_DTYPE, MatchParams, Param

import disparity_ref as DR
import map_ref as M
import tsdf_ref as R

pytestmark = pytest.mark.gpu

INV = R.INVALID
POSE = np.linalg.inv(hostmath.tr2mat([0.013, -0.021, 0.007, 0.31, -0.12, 1.47]))   # a rotation and a translation
LOG2 = 21                                                                         # 2 M slots


def _param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)   # non-integer cu, cv


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want) and got.tobytes() == want.tobytes()


def _clean(st):
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0, st
    return st


def _mixed_map(rng, rows, cols, invalid=0.25):
    """A random mix of valid and invalid pixels, disparities 1 .. 90 px: patches of equal disparity seven pixels wide, broken up by
    single pixels and invalid ones strewn in, so that the runs inside a wave have many lengths."""
    m = np.repeat(rng.integers(16, 90 * 16 + 1, (rows, cols // 7 + 1)), 7, axis=1)[:, :cols]
    single = rng.random((rows, cols)) < 0.3
    m = np.where(single, rng.integers(16, 90 * 16 + 1, (rows, cols)), m).astype(np.int16)
    m[rng.random((rows, cols)) < invalid] = INV
    return m


def _check(tsdf, want, st, tag, min_weights=(1, 2)):
    assert tsdf.stats() == st, (tag, tsdf.stats(), st)
    e = tsdf.entries()
    assert e.dtype == TSDF_ENTRY_DTYPE == R.ENTRY and _same(e, want), tag
    for mw in min_weights:
        c, wc = tsdf.surface(mw), R.crossings(want, mw)
        assert c.dtype == TSDF_CROSSING_DTYPE == R.CROSSING and _same(c, wc), (tag, mw, len(c), len(wc))
        if mw > 1:
            assert _same(tsdf.entries(mw), want[want["weight"] >= mw]), (tag, mw)
    return e


@pytest.mark.parametrize("shape", [(37, 333), (1, 1), (3, 130)])
@pytest.mark.parametrize("trunc", [1, 3, 8])
def test_device_equals_restatement(viso, shape, trunc):
    """(3, 130): runs that cross the wave boundary at columns 63/64 and 127/128, and a short last wave.  voxel 5.0: a whole wave is one
    run; voxel 0.05 at far depth: no two lanes share a voxel."""
    rng = np.random.default_rng(shape[0] * 3 + shape[1] + trunc)
    m = _mixed_map(rng, *shape) if shape != (1, 1) else np.array([[400]], np.int16)
    if m.size > 1:
        m[0, 60:70] = 200            # one run across the first wave boundary
        m.flat[0], m.flat[-1] = 0, 15
    prm = _param()
    n_cross = 0
    for voxel in (0.05, 0.2, 5.0):
        tsdf = libviso_amd.TsdfMap(None, voxel=voxel, trunc_voxels=trunc, capacity_log2=LOG2)
        for name, pose in (("none", None), ("rigid", POSE)):
            want, st = R.fuse([(m, pose)], prm, voxel, trunc, 16, LOG2)
            _clean(st)
            tsdf.clear()
            tsdf.fuse(m, prm, pose=pose)
            _check(tsdf, want, st, (shape, trunc, voxel, name))
            n_cross += len(R.crossings(want))
            p = tsdf.surface_points()
            assert np.array_equal(p.view(np.uint32), R.crossing_points(R.crossings(want), voxel).view(np.uint32))
        tsdf.close()
    assert n_cross > 0 or m.size == 1


def test_full_frame_once(viso):
    rng = np.random.default_rng(1241)
    m = _mixed_map(rng, 376, 1241)
    prm = _param()
    want, st = R.fuse([(m, POSE)], prm, 0.2, 3, 16, 23)
    _clean(st)
    tsdf = libviso_amd.TsdfMap(None, capacity_log2=23)
    tsdf.fuse(m, prm, pose=POSE)
    _check(tsdf, want, st, "full frame", min_weights=(1,))
    print(f"full frame: {st['n_points']} points, {st['n_updates']} updates ({st['n_updates'] / st['n_points']:.2f} a point), {len(want)} voxels")
    tsdf.close()


@pytest.mark.parametrize("method", ["bm", "sgm"])
def test_maps_of_both_methods(viso, method):
    L, Rimg, _ = DR.slanted_pair()
    raw = libviso_amd.stereo_disparity(L, Rimg) if method == "bm" else libviso_amd.stereo_sgm(L, Rimg)
    prm = _param()
    tsdf = libviso_amd.TsdfMap(None, capacity_log2=LOG2)
    for d16 in (raw, libviso_amd.filter_speckles(raw)):
        for pose in (None, POSE):
            want, st = R.fuse([(d16, pose)], prm, capacity_log2=LOG2)
            _clean(st)
            tsdf.clear()
            tsdf.fuse(d16, prm, pose=pose)
            _check(tsdf, want, st, method)
            print(f"{method}: {st['n_points']} points, {st['n_updates']} updates ({st['n_updates'] / max(1, st['n_points']):.2f} a point), "
                  f"{len(want)} voxels, {len(R.crossings(want))} crossings")
    tsdf.close()


def test_degenerate_inputs(viso):
    prm = _param()
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, trunc_voxels=8, capacity_log2=LOG2)
    tsdf.fuse(np.full((37, 333), INV, np.int16), prm)
    assert len(tsdf.entries()) == 0 and len(tsdf.surface()) == 0 and tsdf.surface_points().shape == (0, 3)
    assert tsdf.stats() == dict(n_points=0, n_updates=0, n_out_of_range=0, n_dropped=0, n_occupied=0)
    # points so near (0.25 .. 0.7 m, band 1.6 m) that their first samples have zj <= 0
    rng = np.random.default_rng(6)
    near = rng.integers(16 * 550, 16 * 1500, (5, 70)).astype(np.int16)
    want, st = R.fuse([(near, None)], prm, 0.2, 8, 16, LOG2)
    _clean(st)
    assert (prm.f * prm.base / (near / 16.0) - 16 * 0.1 < 0).all()
    tsdf.fuse(near, prm)
    _check(tsdf, want, st, "near")
    tsdf.close()
    # a pose that pushes part of the samples past 2^30 cells: counted, not inserted
    m = _mixed_map(rng, 37, 333)
    far = POSE.copy(); far[2, 3] += float(R.RANGE) * 0.2 / 1024 - 12.0
    want, st = R.fuse([(m, far)], prm, 0.2, 3, 16, LOG2)
    assert 0 < st["n_out_of_range"] and st["n_updates"] > 0 and st["n_dropped"] == 0
    tsdf = libviso_amd.TsdfMap(None, capacity_log2=LOG2)
    tsdf.fuse(m, prm, pose=far)
    _check(tsdf, want, st, "far")
    # a pose that is not finite is refused, and the map stays as it was
    bad = POSE.copy(); bad[3, 3] = np.nan
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        tsdf.fuse(m, prm, pose=bad)
    assert _same(tsdf.entries(), want)
    tsdf.close()


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


def test_resident_path_partitions_and_lifetime(viso):
    seq = synth.make_subpixel_image_sequence(4, 6, n_kp=500, width=640, height=200)
    prm = seq["param"]
    ctx = libviso_amd.Context(0)
    b = _batch_with_maps(ctx, seq, num_disp=64)
    nf = b.nf
    tsdf = libviso_amd.TsdfMap(ctx, capacity_log2=LOG2)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.fuse_tsdf(tsdf, np.tile(np.eye(4), (nf, 1, 1)))      # no run has computed the maps
    b.set_speckle(max_size=50)
    b.run_images()
    T, valid = _frame_poses(b)
    assert len(valid) >= 2
    vmap = libviso_amd.VoxelMap(ctx, capacity_log2=LOG2)
    b.fuse_disparities(vmap, T)
    before = (b.poses(), [b.matches(w, t) for w in range(3) for t in range(nf)], b.disparities(), vmap.entries())
    maps = [b.disparity(t) for t in range(nf)]
    want, st = R.fuse([(maps[t], T[t]) for t in range(nf)], prm, capacity_log2=LOG2)
    _clean(st)
    # the resident path, all frames in one call
    b.fuse_tsdf(tsdf, T)
    whole = _check(tsdf, want, st, "resident")
    # ... equals fusing the downloaded maps one by one, in reverse order
    one = libviso_amd.TsdfMap(None, capacity_log2=LOG2)
    for t in reversed(range(nf)):
        one.fuse(maps[t], prm, pose=T[t])
    assert _same(one.entries(), whole) and _same(one.surface(), tsdf.surface()) and one.stats() == st
    # partitions: two maps over disjoint frame sets, joined by add_entries
    a, c = libviso_amd.TsdfMap(ctx, capacity_log2=LOG2), libviso_amd.TsdfMap(ctx, capacity_log2=LOG2)
    b.fuse_tsdf(a, T[:2], t0=0, t1=2)
    b.fuse_tsdf(c, T[2:], t0=2)
    part_a = R.fuse([(maps[t], T[t]) for t in range(2)], prm, capacity_log2=LOG2)[0]
    assert _same(a.entries(), part_a)
    part_c = c.entries()
    a.add_entries(part_c)
    assert _same(a.entries(), whole) and _same(R.merge(part_c, part_a), whole) and _same(a.surface(2), R.crossings(whole, 2))
    sa = a.stats()
    assert sa["n_updates"] == st["n_updates"] and sa["n_occupied"] == st["n_occupied"] and sa["n_dropped"] == 0
    # a saved map loaded into an empty one
    c.clear()
    c.add_entries(whole)
    assert _same(c.entries(), whole) and _same(c.surface(), R.crossings(whole))
    # entries that are not voxels of this map are refused before the device
    for field, value in (("weight", 0), ("k", [1 << 20, 0, 0]), ("k", [0, -(1 << 20) - 1, 0]), ("sum", 3 * 1024 + 1), ("sum", -3 * 1024 - 1)):
        bad = np.zeros(1, TSDF_ENTRY_DTYPE)
        bad["weight"] = 1
        bad[field] = value
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            c.add_entries(bad)
    assert _same(c.entries(), whole)
    # the batch's own outputs and the voxel map are byte-identical before and after fusing from it
    after = (b.poses(), [b.matches(w, t) for w in range(3) for t in range(nf)], b.disparities(), vmap.entries())
    for x, y in zip(before[0], after[0]):
        assert np.array_equal(x, y) and x.tobytes() == y.tobytes()
    assert all(np.array_equal(x, y) for x, y in zip(before[1], after[1])) and np.array_equal(before[2], after[2])
    assert before[3].tobytes() == after[3].tobytes() == M.fuse([(maps[t], T[t]) for t in range(nf)], prm, capacity_log2=LOG2)[0].tobytes()
    # argument errors of the resident call
    for bad in (dict(t0=-1, t1=1, poses=T[:2]), dict(t0=0, t1=nf + 1, poses=np.tile(np.eye(4), (nf + 1, 1, 1))), dict(t0=2, t1=2, poses=T[:0])):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b.fuse_tsdf(tsdf, bad["poses"], t0=bad["t0"], t1=bad["t1"])
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.fuse_tsdf(one, T)          # a map of another context
    nan = T.copy(); nan[1, 0, 0] = np.inf
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.fuse_tsdf(tsdf, nan)
    assert _same(tsdf.entries(), whole)
    for v in (one, a, c, vmap):
        v.close()
    # a map that outlives its context: every call answers with a code, and destroy frees it
    b.close(); ctx.close()
    for call in (tsdf.stats, tsdf.entries, tsdf.surface, tsdf.clear, lambda: tsdf.fuse(maps[0], prm), lambda: tsdf.add_entries(whole[:1])):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            call()
    tsdf.close()
    assert tsdf.h is None


def test_overflow_is_an_error_code_and_clear_recovers(viso):
    """A table of 2^10 slots fed a row of 2000 pixels one voxel apart.  The probe loop visits every slot at most once, so the full
    table costs the updates that find no slot 1024 probes each and nothing else."""
    prm = Param.default(base=1.0, f=2.0, cu=0.0, cv=0.0)
    wide = np.full((1, 2000), 16, np.int16)           # d = 1 px: X = x, one voxel of 0.5 m per pixel
    _, st = R.fuse([(wide, None)], prm, 0.5, 1, 1, 10)
    assert st["n_dropped"] > 0 and st["n_occupied"] == 1024
    tsdf = libviso_amd.TsdfMap(None, voxel=0.5, trunc_voxels=1, min_disp16=1, capacity_log2=10)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.fuse(wide, prm)
    got = tsdf.stats()
    assert got["n_dropped"] > 0 and got["n_occupied"] == 1024 and got["n_points"] == 2000 and got["n_updates"] == st["n_updates"]
    small = np.full((1, 100), 16, np.int16)
    for call in (tsdf.entries, tsdf.surface, lambda: tsdf.fuse(small, prm), lambda: tsdf.add_entries(np.zeros(0, TSDF_ENTRY_DTYPE))):
        with pytest.raises(libviso_amd.VisoError, match="-4"):
            call()
    tsdf.clear()
    want, st = R.fuse([(small, None)], prm, 0.5, 1, 1, 10)
    _clean(st)
    tsdf.fuse(small, prm)
    _check(tsdf, want, st, "after clear")
    # add_entries overflows the same way
    many = np.zeros(1500, TSDF_ENTRY_DTYPE)
    many["k"][:, 0] = np.arange(1500) + 500
    many["weight"], many["sum"] = 1, -7
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.add_entries(many)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.entries()
    tsdf.clear()
    tsdf.add_entries(many[:1024])          # exactly full: no drop
    assert _same(tsdf.entries(), R.merge(many[:1024])) and tsdf.stats()["n_occupied"] == 1024 and len(tsdf.surface()) == 0
    tsdf.close()


@pytest.mark.parametrize("d16", [325, 115])
def test_fronto_parallel_wall_under_a_rigid_pose(viso, d16):
    """The wall of test_tsdf_cpu.test_fronto_parallel_wall seen through a rigid pose.  In the camera frame the argument is the same up
    to rounding: a voxel's q is floor((Z0 - zc) / s) for every pixel that touches it, so its mean is that integer; two voxels
    adjacent along an axis differ in zc by 1024 s R[axis][2] (R the rotation), so the interpolated crossing lies where Z0 - zc is zero
    up to the two floors: its depth in the camera frame, (R^T (p - t))_z, is within 2 s of Z0.  On top come the roundings of the three
    coordinates of p to float32, each at most half an ulp, |p_i| 2^-24, which the rotation back weighs with |R[i][2]| <= 1."""
    prm = _param()
    m = np.full((37, 333), d16, np.int16)
    voxel = 0.2
    want, st = R.fuse([(m, POSE)], prm, voxel, 3, 16, LOG2)
    _clean(st)
    tsdf = libviso_amd.TsdfMap(None, voxel=voxel, capacity_log2=LOG2)
    tsdf.fuse(m, prm, pose=POSE)
    _check(tsdf, want, st, "wall")
    p = tsdf.surface_points().astype(np.float64)
    tsdf.close()
    assert len(p) > 0
    Z0 = prm.f * prm.base / (d16 / 16.0)
    s = voxel / 1024.0
    depth = (p - POSE[:3, 3]) @ POSE[:3, 2]
    err = np.abs(depth - Z0)
    bound = 2.0 * s + (np.abs(p) * 2.0 ** -24) @ np.abs(POSE[:3, 2])
    print(f"disp16 {d16}: {len(p)} crossings, worst |depth - Z0| = {err.max() / s:.3f} s, smallest margin {(bound - err).min() / s:.3f} s")
    assert (err <= bound).all()


def _chained_poses(nf=5):
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


def test_slanted_pair_once_and_from_chained_poses(viso):
    """slanted_pair renders the plane d*(x, y) = a + b x + c y in disparity space: n . P = f base in space with
    n = (b f, c f, a + b cu + c cv) (test_gpu_map.test_centroids_of_the_slanted_pair_lie_on_its_plane).  Seen from a camera at pose
    T = (R, t) the same map places it at n' . (P' - t) = f base with n' = R n.

    Equality with the restatement is the assertion.  The distances of the crossings from the plane are printed beside those of the
    voxel map's centroids on the same input, and no bound on them is asserted: none has been derived.  (A crossing interpolates
    between two voxel means, each a mean of floored, truncated projective distances along the viewing direction of several pixels;
    near the rim of the band the truncation biases a mean, and the matcher's own error enters as it does for the centroids.)"""
    L, Rimg, dtrue = DR.slanted_pair()
    raw = libviso_amd.stereo_disparity(L, Rimg)
    prm = _param()
    f, cu, cv, base = prm.f, prm.cu, prm.cv, prm.base
    rows, cols = raw.shape
    a = dtrue[0, 0]; b = (dtrue[0, -1] - dtrue[0, 0]) / (cols - 1); c = (dtrue[-1, 0] - dtrue[0, 0]) / (rows - 1)
    n = np.array([b * f, c * f, a + b * cu + c * cv])

    def dist(P, pose):
        P = P.astype(np.float64)
        if pose is None:
            return np.abs(P @ n - f * base) / np.linalg.norm(n)
        return np.abs((P - pose[:3, 3]) @ (pose[:3, :3] @ n) - f * base) / np.linalg.norm(n)

    # once, from one pose
    for pose in (None, POSE):
        want, st = R.fuse([(raw, pose)], prm, capacity_log2=LOG2)
        _clean(st)
        tsdf = libviso_amd.TsdfMap(None, capacity_log2=LOG2)
        tsdf.fuse(raw, prm, pose=pose)
        _check(tsdf, want, st, "slanted")
        vmap = libviso_amd.VoxelMap(None, capacity_log2=LOG2)
        vmap.fuse(raw, prm, pose=pose)
        ds, dc = dist(tsdf.surface_points(), pose), dist(vmap.centroids(), pose)
        print(f"pose {'none' if pose is None else 'rigid'}: {len(ds)} crossings, distance from the plane: median {np.median(ds):.4f} m, "
              f"max {ds.max():.4f} m; {len(dc)} centroids: median {np.median(dc):.4f} m, max {dc.max():.4f} m")
        tsdf.close(); vmap.close()
    # the same map fused under each of five chained poses into one map: five copies of the plane
    chained = _chained_poses()
    frames = [(raw, T) for T in chained]
    want, st = R.fuse(frames, prm, capacity_log2=LOG2)
    _clean(st)
    tsdf = libviso_amd.TsdfMap(None, capacity_log2=LOG2)
    for m, T in frames:
        tsdf.fuse(m, prm, pose=T)
    _check(tsdf, want, st, "chained")
    p = tsdf.surface_points(2)
    nearest = np.min([dist(p, T) for T in chained], axis=0)
    print(f"{len(chained)} chained poses: {len(want)} voxels, {len(p)} crossings at min_weight 2, distance from the nearest of the planes: "
          f"median {np.median(nearest):.4f} m, max {nearest.max():.4f} m")
    tsdf.close()
