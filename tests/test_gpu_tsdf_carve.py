"""The TSDF fuse options on the device (include/viso_hip.h, "TSDF fuse options"; tsdf_carve_fuse_kernel and tsdf_gray_carve_fuse_kernel
of libviso_amd/csrc/tsdf.hip) against their numpy restatement (tests/carve_ref.py), bit for bit on the sorted entries, on the
crossings and on every counter; the ghost that carving removes, in the crossings and in a render; the resident path; the defaults;
the tool.

Input condition of the bit-exact cases, asserted first: the restatement itself reports n_out_of_range == 0 and n_dropped == 0."""
import ctypes as C
import os

import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map, hostmath, synth
from libviso_amd.abi import TSDF_CROSSING_DTYPE, TSDF_ENTRY_DTYPE, TSDF_GRAY_ENTRY_DTYPE, MatchParams, Param

import carve_ref as CR
import gray_ref as G
import render_ref as RR
import tsdf_ref as R
from test_tsdf_carve_cpu import GHOST_TRUNC, GHOST_VOXEL, check_ghost, ghost_frames

pytestmark = pytest.mark.gpu

INV = R.INVALID
POSE = np.linalg.inv(hostmath.tr2mat([0.013, -0.021, 0.007, 0.31, -0.12, 1.47]))   # a rotation and a translation
OPTIONS = {"carve": dict(carve_voxels=6), "weights": dict(weight_shift=12, weight_max=255),
           "both": dict(carve_voxels=6, weight_shift=12, weight_max=255)}


def _param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)   # non-integer cu, cv


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _clean(st):
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0, st
    return st


def _log2_for(n_voxels):
    """A table at most half full."""
    return max(10, int(np.ceil(np.log2(max(1, 2 * n_voxels)))))


def _mixed_map(rng, rows, cols, invalid=0.25):
    """tests/test_gpu_tsdf.py's: patches of equal disparity seven pixels wide, broken up by single pixels and invalid ones, so that
    the runs inside a wave have many lengths and, with weights, lanes of one run carry different w."""
    m = np.repeat(rng.integers(16, 90 * 16 + 1, (rows, cols // 7 + 1)), 7, axis=1)[:, :cols]
    single = rng.random((rows, cols)) < 0.3
    m = np.where(single, rng.integers(16, 90 * 16 + 1, (rows, cols)), m).astype(np.int16)
    m[rng.random((rows, cols)) < invalid] = INV
    return m


def _check(tsdf, want, st, tag):
    """Entries, crossings at min_weight 1 and 2 and all counters of the device map against the restatement's."""
    assert tsdf.stats() == st, (tag, tsdf.stats(), st)
    e = tsdf.entries()
    assert e.dtype == TSDF_ENTRY_DTYPE == R.ENTRY and _same(e, G.plain(want) if want.dtype == G.ENTRY else want), tag
    for mw in (1, 2):
        c, wc = tsdf.surface(mw), R.crossings(e, mw)
        assert c.dtype == TSDF_CROSSING_DTYPE == R.CROSSING and _same(c, wc), (tag, mw, len(c), len(wc))
    return e


def _device(frames, prm, voxel, trunc, min_disp16, o, tag, gray=False):
    """The restatement of `frames` and a device map of the smallest capacity that holds it twice, fused frame by frame and checked."""
    want, st = CR.fuse(frames, prm, voxel, trunc, min_disp16, gray=gray, **o)
    log2 = _log2_for(len(want))
    st = dict(st, n_occupied=min(len(want), 1 << log2))
    _clean(st)
    tsdf = libviso_amd.TsdfMap(None, gray=gray, voxel=voxel, trunc_voxels=trunc, min_disp16=min_disp16, capacity_log2=log2, **o)
    for fr in frames:
        if gray:
            tsdf.fuse(fr[0], prm, pose=fr[2], image=fr[1])
        else:
            tsdf.fuse(fr[0], prm, pose=fr[1])
    _check(tsdf, want, st, tag)
    if gray:
        ge = tsdf.entries(gray=True)
        assert ge.dtype == TSDF_GRAY_ENTRY_DTYPE == G.ENTRY and _same(ge, want), tag
    return tsdf, want, st


@pytest.mark.parametrize("options", sorted(OPTIONS))
@pytest.mark.parametrize("shape", [(1, 1), (3, 130), (37, 333)])
def test_device_equals_restatement(viso, shape, options):
    """(3, 130): runs that cross the wave boundary at columns 63/64 and 127/128, and a short last wave.  voxel 5.0: a whole wave is one
    run; voxel 0.05 at far depth: no two lanes share a voxel."""
    o = OPTIONS[options]
    rng = np.random.default_rng(shape[0] * 3 + shape[1])
    m = _mixed_map(rng, *shape) if shape != (1, 1) else np.array([[400]], np.int16)
    if m.size > 1:
        m[0, 60:70] = 200            # one run across the first wave boundary
        m.flat[0], m.flat[-1] = 0, 15
    prm = _param()
    n_cross = 0
    for trunc in (1, 3):
        for voxel in (0.05, 0.2, 5.0):
            for name, pose in (("none", None), ("rigid", POSE)):
                tsdf, want, st = _device([(m, pose)], prm, voxel, trunc, 16, o, (shape, options, trunc, voxel, name))
                n_cross += len(R.crossings(want))
                if "weight_shift" in o and m.size > 1:
                    assert int(want["weight"].sum()) > st["n_updates"]      # the weights are in play
                tsdf.close()
    assert n_cross > 0 or m.size == 1


def test_named_waves(viso):
    """The cases a sum or the loop's start can go wrong at."""
    # every lane of a wave in one voxel, at the largest weight and the clamped q, T = 8: voxel 5, d16 = 1024 (w = 256 -> 255) at
    # Z = 100 m, 12 carved samples of which the nearest lie more than 40 m in front of the point: the run's sum of w (q + T 1024)
    # is 64 x 255 x 16384, the bound the 32-bit scan is sized for
    prm = Param.default(base=1.0, f=6400.0, cu=-1.0, cv=-1.0)
    m = np.full((1, 64), 1024, np.int16)
    o = dict(carve_voxels=6, weight_shift=12, weight_max=255)
    tsdf, want, st = _device([(m, None)], prm, 5.0, 8, 16, o, "one run at the bound")
    assert st["n_updates"] == 64 * len(want) and (want["weight"] == 64 * 255).all() and want["sum"].max() == 64 * 255 * 8192
    tsdf.close()
    image = np.full((1, 64), 255, np.uint8)
    tsdf, want, _ = _device([(m, image, None)], prm, 5.0, 8, 16, o, "one run at the bound, gray", gray=True)
    assert (want["gray"] == 64 * 255 * 255).all()
    tsdf.close()
    # pixels nearer than the carved length (0.5 m < 6 x 0.2 m) beside far ones in every wave: the wave starts where its farthest
    # lane needs it, the near lanes skip their samples at zj <= 0
    prm = _param()
    m = np.full((2, 130), 100, np.int16)
    m[:, ::2] = 12401
    assert prm.f * prm.base / (12401 / 16.0) < 0.51 < 6 * 0.2
    for name, pose in (("none", None), ("rigid", POSE)):
        _device([(m, pose)], prm, 0.2, 3, 16, OPTIONS["both"], ("near and far", name))[0].close()
    # carve_near between two samples of a pixel: Z = 3.1 m, samples every 0.1 m, carve_near 1.234; and on the sample itself
    m = np.full((3, 70), 2000, np.int16)
    Z = prm.f * prm.base / (2000 / 16.0)
    for near in (1.234, float(Z + np.float64(-15) * np.float64(0.1))):
        e_near = _device([(m, POSE)], prm, 0.2, 3, 16, dict(carve_voxels=20, carve_near=near), ("carve_near", near))
        e_all = CR.fuse([(m, POSE)], prm, 0.2, 3, 16, carve_voxels=20)[0]
        assert len(e_near[1]) < len(e_all)
        e_near[0].close()


@pytest.mark.parametrize("shape", [(3, 130), (37, 333)])
def test_gray_map(viso, shape):
    rng = np.random.default_rng(shape[1])
    m = _mixed_map(rng, *shape)
    image = rng.integers(0, 256, shape).astype(np.uint8)
    prm = _param()
    for trunc, voxel, pose in ((3, 0.2, POSE), (1, 5.0, None), (3, 0.05, None)):
        gmap, want, st = _device([(m, image, pose)], prm, voxel, trunc, 16, OPTIONS["both"], (shape, trunc, voxel), gray=True)
        pmap, pwant, pst = _device([(m, pose)], prm, voxel, trunc, 16, OPTIONS["both"], (shape, trunc, voxel, "plain"))
        assert _same(gmap.entries(), pmap.entries()) and pst == st and (want["gray"] <= 255 * want["weight"].astype(np.uint64)).all()
        gmap.close(); pmap.close()


def test_ghost_scene(viso):
    prm, frames, d5, d10 = ghost_frames()
    shape = frames[0][0].shape
    entries = {}
    for carve, seen in ((0, d5), (28, d10)):
        tsdf, want, st = _device(frames, prm, GHOST_VOXEL, GHOST_TRUNC, 16, dict(carve_voxels=carve), ("ghost", carve))
        entries[carve] = tsdf.entries()
        # what a camera at the identity pose sees at the patch's centre: the patch without carving, the wall behind it with
        d = tsdf.render(prm, shape, None, max_depth=40.0, min_weight=1)
        assert d[12, 96] == seen and d[2, 5] == d10, (carve, d[12, 96], d[2, 5])
        assert _same(d, RR.render(want, GHOST_VOXEL, prm, shape, None, 40.0, 1)[0])
        print(f"C = {carve}: {st['n_updates'] / st['n_points']:.2f} updates a point, {len(want)} voxels")
        tsdf.close()
    check_ghost(entries[0], entries[28])


def _batch_with_maps(ctx, seq, **disp):
    nf, cap = seq["kp"].shape[0], seq["kp"].shape[2]
    b = libviso_amd.Batch(ctx, nf, cap)
    b.upload_images(seq["images"], seq["kp"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=3)
    b.set_disparity(**disp)
    return b


def test_resident_path_partitions_and_order(viso):
    seq = synth.make_subpixel_image_sequence(4, 4, n_kp=500, width=640, height=200)
    prm = seq["param"]
    ctx = libviso_amd.Context(0)
    b = _batch_with_maps(ctx, seq, num_disp=64)
    nf = b.nf
    b.run_images()
    T = np.array([np.linalg.inv(hostmath.tr2mat([0.0, 0.004 * t, 0.0, 0.02 * t, 0.0, -0.3 * t])) for t in range(nf)])
    maps = [b.disparity(t) for t in range(nf)]
    o = OPTIONS["both"]
    want, st = CR.fuse([(maps[t], T[t]) for t in range(nf)], prm, **o)
    log2 = _log2_for(len(want))
    st = _clean(dict(st, n_occupied=len(want)))
    assert st["n_points"] > 1000
    # the resident path with the map's options, all frames in one call
    tsdf = libviso_amd.TsdfMap(ctx, capacity_log2=log2, **o)
    b.fuse_tsdf(tsdf, T)
    whole = _check(tsdf, want, st, "resident")
    # ... equals the host path on the downloaded maps, in reverse order
    one = libviso_amd.TsdfMap(ctx, capacity_log2=log2)
    one.fuse_options = o
    for t in reversed(range(nf)):
        one.fuse(maps[t], prm, pose=T[t])
    assert _same(one.entries(), whole) and _same(one.surface(), tsdf.surface()) and one.stats() == st
    # partitions joined by add_entries
    a, c = libviso_amd.TsdfMap(ctx, capacity_log2=log2, **o), libviso_amd.TsdfMap(ctx, capacity_log2=log2, **o)
    b.fuse_tsdf(a, T[:1], t0=0, t1=1)
    b.fuse_tsdf(c, T[1:], t0=1)
    assert _same(a.entries(), CR.fuse([(maps[0], T[0])], prm, **o)[0])
    a.add_entries(c.entries())
    assert _same(a.entries(), whole) and _same(a.surface(2), R.crossings(whole, 2))
    sa = a.stats()
    assert sa["n_occupied"] == st["n_occupied"] and sa["n_dropped"] == 0
    # the options persist across clear, and a gray map takes them on the resident path too
    tsdf.clear()
    assert tsdf.fuse_options == dict(carve_voxels=6, weight_shift=12, weight_max=255, carve_near=0.0)
    b.fuse_tsdf(tsdf, T)
    assert _same(tsdf.entries(), whole)
    gmap = libviso_amd.TsdfMap(ctx, gray=True, capacity_log2=log2, **o)
    b.fuse_tsdf(gmap, T)
    gwant = CR.fuse([(maps[t], seq["images"][t, 0], T[t]) for t in range(nf)], prm, gray=True, **o)[0]
    assert _same(gmap.entries(gray=True), gwant) and _same(gmap.entries(), whole)
    for v in (tsdf, one, a, c, gmap):
        v.close()
    b.close(); ctx.close()


def test_defaults_and_refusals(viso):
    rng = np.random.default_rng(9)
    m = _mixed_map(rng, 37, 333)
    prm = _param()
    want, st = R.fuse([(m, POSE)], prm, capacity_log2=18)
    _clean(st)
    plain = libviso_amd.TsdfMap(None, capacity_log2=18)
    explicit = libviso_amd.TsdfMap(None, capacity_log2=18, carve_voxels=0, weight_shift=None, weight_max=255, carve_near=0.0)
    assert plain.fuse_options == explicit.fuse_options == dict(carve_voxels=0, weight_shift=None, weight_max=255, carve_near=0.0)
    reset = libviso_amd.TsdfMap(None, capacity_log2=18, **OPTIONS["both"])
    reset.fuse_options = {}                          # back to the defaults
    for t in (plain, explicit, reset):
        t.fuse(m, prm, pose=POSE)
        assert _same(t.entries(), want) and t.stats() == st and _same(t.surface(), R.crossings(want))
    # values out of range are refused and leave the options as they were, on a plain and on a gray map
    gmap = libviso_amd.TsdfMap(None, gray=True, capacity_log2=10, carve_voxels=3, carve_near=0.5)
    reset.fuse_options = dict(carve_voxels=3, carve_near=0.5)
    for t in (reset, gmap):
        for bad in (dict(carve_voxels=1025), dict(carve_voxels=-1), dict(weight_shift=31), dict(weight_shift=3, weight_max=0),
                    dict(weight_shift=3, weight_max=256), dict(carve_near=-1.0), dict(carve_near=float("nan"))):
            with pytest.raises(libviso_amd.VisoError, match="-1"):
                t.fuse_options = bad
            assert t.fuse_options == dict(carve_voxels=3, weight_shift=None, weight_max=255, carve_near=0.5), bad
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        libviso_amd.TsdfMap(None, capacity_log2=10, carve_voxels=2000)
    # a destroyed handle answers with a code
    h = plain.h
    for t in (plain, explicit, reset, gmap):
        t.close()
    c, s, m, n = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_double()
    assert viso.viso_tsdf_set_fuse_options(h, 0, -1, 255, 0.0) == -1
    assert viso.viso_tsdf_get_fuse_options(h, C.byref(c), C.byref(s), C.byref(m), C.byref(n)) == -1


def test_tool_carves(viso, tmp_path):
    """fuse_map --surface --carve 28 on a runner's directory made from the ghost scene writes the restatement's PLY; without the
    flag, the PLY of before the flag existed."""
    prm, frames, _, _ = ghost_frames()
    d = tmp_path / "disp"
    d.mkdir()
    for i, (m, _) in enumerate(frames):
        fuse_map.write_disparity_png(str(d / ("%06d.png" % i)), m)
    poses, calib = str(tmp_path / "poses.txt"), str(tmp_path / "calib.txt")
    fuse_map.write_poses(poses, [np.eye(4)] * len(frames))
    P0 = [prm.f, 0.0, prm.cu, 0.0, 0.0, prm.f, prm.cv, 0.0, 0.0, 0.0, 1.0, 0.0]
    P1 = list(P0)
    P1[3] = -prm.f * prm.base
    with open(calib, "w") as f:
        f.write("P0: " + " ".join("%.17g" % v for v in P0) + "\nP1: " + " ".join("%.17g" % v for v in P1) + "\n")
    f_, cu, cv, base = fuse_map.read_calib(calib)
    read = Param.default(base=base, f=f_, cu=cu, cv=cv)
    maps = [fuse_map.read_disparity_png(str(d / n)) for n in sorted(os.listdir(str(d)))]
    assert all(np.array_equal(a, b[0]) for a, b in zip(maps, frames))
    outs = {}
    for tag, args in (("plain", []), ("carve", ["--carve", "28"]), ("all", ["--carve", "28", "--carve-near", "1.0", "--depth-weights", "12,200"])):
        out = str(tmp_path / (tag + ".ply"))
        assert fuse_map.main([str(d), poses, calib, out, "--surface", "--capacity-log2", "12"] + args) == 0
        outs[tag] = open(out, "rb").read()
    fr = [(m, np.eye(4)) for m in maps]
    assert outs["plain"] == R.ply_bytes(R.crossings(R.fuse(fr, read, GHOST_VOXEL, GHOST_TRUNC, 16, 12)[0]), GHOST_VOXEL)
    want, st = CR.fuse(fr, read, GHOST_VOXEL, GHOST_TRUNC, 16, 12, carve_voxels=28)
    _clean(st)
    assert outs["carve"] == R.ply_bytes(R.crossings(want), GHOST_VOXEL) and outs["carve"] != outs["plain"]
    want, st = CR.fuse(fr, read, GHOST_VOXEL, GHOST_TRUNC, 16, 12, carve_voxels=28, carve_near=1.0, weight_shift=12, weight_max=200)
    _clean(st)
    assert outs["all"] == R.ply_bytes(R.crossings(want), GHOST_VOXEL)
