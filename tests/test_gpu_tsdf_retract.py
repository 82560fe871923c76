"""The TSDF retract on the device (include/viso_hip.h, "TSDF retract"; the take kernels of libviso_amd/csrc/tsdf.hip, the check and the
mark of voxel_hash.h) against its numpy restatement (tests/retract_ref.py) and against a fresh device map that never saw the frame:
bit for bit on the sorted entries, the gray entries, the crossings and every counter; to the empty map and back; the probe clusters
of small and of full tables; every refusal leaving the map as it was; the argument refusals; the move; the tool.

Input condition of every case, asserted first on the restatement alone (test_tsdf_retract_cpu.fuse): n_out_of_range == 0,
n_dropped == 0, and no weight wraps."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map, hostmath, synth
from libviso_amd.abi import TSDF_CROSSING_DTYPE, TSDF_ENTRY_DTYPE, TSDF_GRAY_ENTRY_DTYPE, MatchParams

import carve_ref as CR
import evict_ref as E
import gray_ref as G
import retract_ref as RT
import tsdf_ref as R
from test_tsdf_retract_cpu import MIN_DISP16, OPTIONS, POSES, SHAPES, TRUNC, VOXEL, fuse, param, refusal_cases, retract, same, scene

pytestmark = pytest.mark.gpu


def _log2_for(n_voxels):
    """A table at most half full."""
    return max(10, int(np.ceil(np.log2(max(1, 2 * n_voxels)))))


def _map(gray, o, log2, voxel=VOXEL, ctx=None):
    return libviso_amd.TsdfMap(ctx, gray=gray, voxel=voxel, trunc_voxels=TRUNC, min_disp16=MIN_DISP16, capacity_log2=log2, **o)


def _fuse(tsdf, frames):
    for fr in frames:
        if tsdf.gray:
            tsdf.fuse(fr[0], param(), pose=fr[2], image=fr[1])
        else:
            tsdf.fuse(fr[0], param(), pose=fr[1])


def _retract(tsdf, fr):
    return tsdf.retract(fr[0], param(), pose=fr[2], image=fr[1]) if tsdf.gray else tsdf.retract(fr[0], param(), pose=fr[1])


def _state(tsdf):
    """Everything a refused call must leave as it was: the entries (a gray map's with their gray sums) and the counters."""
    return tsdf.entries(gray=tsdf.gray).tobytes(), tsdf.stats()


def _check(tsdf, want, st, tag):
    """Entries, gray entries, crossings at min_weight 1 and 2 and all five counters of the device map against the restatement's."""
    assert tsdf.stats() == st, (tag, tsdf.stats(), st)
    e = tsdf.entries()
    assert e.dtype == TSDF_ENTRY_DTYPE == R.ENTRY and same(e, G.plain(want) if want.dtype == G.ENTRY else want), tag
    if tsdf.gray:
        ge = tsdf.entries(gray=True)
        assert ge.dtype == TSDF_GRAY_ENTRY_DTYPE == G.ENTRY and same(ge, want), tag
    for mw in (1, 2):
        c, wc = tsdf.surface(mw), R.crossings(e, mw)
        assert c.dtype == TSDF_CROSSING_DTYPE == R.CROSSING and same(c, wc), (tag, mw, len(c), len(wc))
    return e


def _same_maps(a, b, tag):
    """Two device maps hold the same table, as far as any getter can tell."""
    assert a.stats() == b.stats(), (tag, a.stats(), b.stats())
    assert same(a.entries(gray=a.gray), b.entries(gray=b.gray)), tag
    for mw in (1, 2):
        assert same(a.surface(mw), b.surface(mw)), (tag, mw)


@pytest.mark.parametrize("options", sorted(OPTIONS))
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_retract_is_bit_exact(viso, shape, gray, options):
    o = OPTIONS[options]
    A, B, C_ = scene(shape, gray)
    e, st = fuse([A, B, C_], gray, o)
    want, wst, wrep, ok = retract(e, st, [B], gray, o)
    assert ok and same(want, fuse([A, C_], gray, o)[0])
    log2 = _log2_for(len(e))
    tsdf, fresh = _map(gray, o, log2), _map(gray, o, log2)
    _fuse(tsdf, [A, B, C_])
    _check(tsdf, e, st, (shape, gray, options, "fused"))
    rep = _retract(tsdf, B)
    assert RT.same_report(rep, wrep) and rep["n_underflow"] == 0, (rep, wrep)
    _check(tsdf, want, wst, (shape, gray, options, "retracted"))
    _fuse(fresh, [A, C_])
    _same_maps(tsdf, fresh, (shape, gray, options))
    tsdf.close(); fresh.close()


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_to_empty_and_back(viso, shape, gray):
    o = OPTIONS["both"]
    frames = scene(shape, gray)
    e, st = fuse(frames, gray, o)
    a_alone, ast = fuse(frames[:1], gray, o)
    tsdf = _map(gray, o, _log2_for(len(e)))
    _fuse(tsdf, frames)
    freed = sum(_retract(tsdf, frames[k])["n_freed"] for k in (2, 0, 1))
    assert freed == len(e) and len(tsdf.entries()) == 0
    assert tsdf.stats() == dict(n_points=0, n_updates=0, n_out_of_range=0, n_occupied=0, n_dropped=0)
    _fuse(tsdf, frames[:1])
    _check(tsdf, a_alone, ast, (shape, gray, "A again"))
    tsdf.close()


@pytest.mark.parametrize("log2", [None, 10])
def test_clusters_survive_in_a_small_table(viso, log2):
    """A table about half full (as _log2_for sizes it) and one of 2^10 slots that is 87 % full, so that probe clusters are long and
    a slot that stayed behind, or a survivor that no probe reaches any more, shows in what follows the retract."""
    gray = True
    shape, voxel, o = ((37, 333), VOXEL, OPTIONS["both"]) if log2 is None else ((3, 130), 0.5, OPTIONS["default"])
    A, B, C_ = scene(shape, gray)
    e, st = fuse([A, B, C_], gray, o, voxel)
    want, wst, wrep, ok = retract(e, st, [B], gray, o, voxel)
    assert ok and wrep["n_freed"] > 0
    log2 = log2 or _log2_for(len(e))
    assert (1 << log2) // 8 < len(e) < (1 << log2)
    tsdf, fresh = _map(gray, o, log2, voxel), _map(gray, o, log2, voxel)
    _fuse(tsdf, [A, B, C_])
    assert RT.same_report(_retract(tsdf, B), wrep)
    _check(tsdf, want, wst, "retracted")
    _fuse(fresh, [A, C_])
    # what reads the table through probes: the mesh with its vertices' gray, and a render
    for got, ref in zip(tsdf.mesh(1, gray=True), fresh.mesh(1, gray=True)):
        assert same(got, ref)
    view = (37, 333)
    for got, ref in zip(tsdf.render(param(), view, POSES[1], max_depth=60.0, min_weight=1, weights=True, gray=True),
                        fresh.render(param(), view, POSES[1], max_depth=60.0, min_weight=1, weights=True, gray=True)):
        assert same(got, ref)
    # every surviving key is still found: fusing B again claims exactly the freed voxels again
    _fuse(tsdf, [B])
    _check(tsdf, e, st, "B again")
    assert RT.same_report(_retract(tsdf, B), wrep)
    # an eviction behind a retract lists what the restatement lists
    lo, hi = E.box_around(POSES[1][:3, 3] + POSES[1][:3, :3] @ np.array([0.0, 0.0, 12.0]), 6.0, voxel)
    kept, gone = E.split(want, lo, hi)
    assert len(kept) and len(gone)
    assert same(tsdf.evict((lo, hi)), gone)
    _check(tsdf, kept, dict(wst, n_occupied=len(kept)), "evicted")
    tsdf.close(); fresh.close()


@pytest.mark.parametrize("gray", [False, True])
def test_table_without_an_empty_slot(viso, gray):
    """A and B in a table of 2^10 slots, filled to exactly 1024 voxels with voxels far from the scene: the retract of B has no
    cluster head to rebuild from and goes the eviction's other way."""
    voxel, o = 0.5, OPTIONS["default"]
    A, B, _ = scene((3, 130), gray)
    e, st = fuse([A, B], gray, o, voxel)
    n_fill = 1024 - len(e)
    assert 0 < n_fill < 1024
    fill = np.zeros(n_fill, G.ENTRY if gray else R.ENTRY)
    fill["k"] = np.stack([20000 + 37 * np.arange(n_fill), np.full(n_fill, -30000), 11 * np.arange(n_fill) - 9000], axis=1)
    fill["weight"], fill["sum"] = 1 + np.arange(n_fill) % 5, 100 - np.arange(n_fill)
    merge = G.merge if gray else R.merge
    full = merge(e, fill)
    fst = dict(st, n_updates=st["n_updates"] + int(fill["weight"].sum()), n_occupied=1024)
    want, wst, wrep, ok = retract(full, fst, [B], gray, o, voxel)
    assert ok and 0 < wrep["n_freed"] < len(e) and len(full) == 1024
    tsdf = _map(gray, o, 10, voxel)
    _fuse(tsdf, [A, B])
    tsdf.add_entries(fill)
    _check(tsdf, full, fst, "full")
    rep = _retract(tsdf, B)
    assert RT.same_report(rep, wrep)
    _check(tsdf, want, wst, "retracted")
    assert tsdf.stats()["n_occupied"] == 1024 - rep["n_freed"]
    # every filler and every voxel of A is still found: the same entries come back through probes
    back = _map(gray, o, 10, voxel)
    back.add_entries(tsdf.entries(gray=gray))
    tsdf.add_entries(want)
    back.add_entries(want)
    assert same(tsdf.entries(gray=gray), back.entries(gray=gray)) and tsdf.stats()["n_occupied"] == len(want)
    tsdf.close(); back.close()


def _refused_on_device(tsdf, frame, wrep, tag):
    before = _state(tsdf)
    with pytest.raises(libviso_amd.VisoError, match="failed with -1: .*n_missing") as err:
        _retract(tsdf, frame)
    assert RT.same_report(err.value.report, wrep), (tag, err.value.report, wrep)
    assert _state(tsdf) == before, tag


@pytest.mark.parametrize("gray", [False, True])
def test_refusals_leave_the_map_bit_identical(viso, gray):
    for name, frames, o, frame, ro, causes in refusal_cases(gray):
        e, st = fuse(frames, gray, o)
        _, _, wrep, ok = retract(e, st, [frame], gray, ro)
        assert not ok and any(wrep[c] for c in causes), (name, wrep)      # refused by the restatement, for the expected cause
        tsdf = _map(gray, o, _log2_for(len(e)))
        _fuse(tsdf, frames)
        tsdf.fuse_options = ro
        _refused_on_device(tsdf, frame, wrep, name)
        tsdf.close()
    A, B, C_ = scene((37, 333), gray)
    e, st = fuse([A, B, C_], gray, {})
    tsdf = _map(gray, {}, _log2_for(len(e)))
    _fuse(tsdf, [A, B, C_])
    # B twice
    once, ost, _, ok = retract(e, st, [B], gray, {})
    _, _, wrep, ok2 = retract(once, ost, [B], gray, {})
    assert ok and not ok2 and wrep["n_missing"] > 0
    _retract(tsdf, B)
    _refused_on_device(tsdf, B, wrep, "B twice")
    # B after an eviction that removed part of it
    _fuse(tsdf, [B])
    lo, hi = E.box_around(POSES[1][:3, 3] + POSES[1][:3, :3] @ np.array([0.0, 0.0, 12.0]), 6.0, VOXEL)
    kept, gone = E.split(e, lo, hi)
    _, _, wrep, ok = retract(kept, dict(st, n_occupied=len(kept)), [B], gray, {})
    assert not ok and wrep["n_missing"] > 0 and len(gone)
    assert same(tsdf.evict((lo, hi)), gone)
    _refused_on_device(tsdf, B, wrep, "B after an eviction")
    tsdf.close()


def test_argument_refusals(viso):
    """Refused with a code before any device work: the report stays as it was."""
    prm = param()
    A, B, _ = scene((3, 130), True)
    m, image, pose = B
    plain, gmap = _map(False, {}, 12), _map(True, {}, 12)
    plain.fuse(m, prm, pose=pose)
    gmap.fuse(m, prm, pose=pose, image=image)
    states = _state(plain), _state(gmap)
    with pytest.raises(ValueError):
        plain.retract(m, prm, pose=pose, image=image)
    with pytest.raises(ValueError):
        gmap.move(m, prm, pose, POSES[0])
    rep = libviso_amd.abi.TsdfRetractReport(*[7] * 6)
    d, im, T = (np.ascontiguousarray(v) for v in (m, image, pose))
    dp, ip, Tp = (libviso_amd.abi.ptr(d, libviso_amd.abi.C.c_int16), libviso_amd.abi.ptr(im, libviso_amd.abi.C.c_uint8),
                  libviso_amd.abi.ptr(T, libviso_amd.abi.C.c_double))
    byref = libviso_amd.abi.C.byref
    # the kinds do not mix
    assert viso.viso_tsdf_retract(gmap.h, dp, 3, 130, byref(prm), Tp, rep.words()) == -1
    assert viso.viso_tsdf_retract_gray(plain.h, dp, ip, 3, 130, byref(prm), Tp, rep.words()) == -1
    assert viso.viso_tsdf_move(gmap.h, dp, 3, 130, byref(prm), Tp, Tp, rep.words()) == -1
    assert viso.viso_tsdf_move_gray(plain.h, dp, ip, 3, 130, byref(prm), Tp, Tp, rep.words()) == -1
    # null pointers and sizes
    assert viso.viso_tsdf_retract(plain.h, None, 3, 130, byref(prm), Tp, rep.words()) == -1
    assert viso.viso_tsdf_retract(plain.h, dp, 3, 130, None, Tp, rep.words()) == -1
    assert viso.viso_tsdf_retract(plain.h, dp, 0, 130, byref(prm), Tp, rep.words()) == -1
    assert viso.viso_tsdf_retract_gray(gmap.h, dp, None, 3, 130, byref(prm), Tp, rep.words()) == -1
    # a pose that is not finite: the retract's, and either pose of a move
    bad = T.copy()
    bad[1, 2] = np.nan
    bp = libviso_amd.abi.ptr(bad, libviso_amd.abi.C.c_double)
    assert viso.viso_tsdf_retract(plain.h, dp, 3, 130, byref(prm), bp, rep.words()) == -1
    assert viso.viso_tsdf_move(plain.h, dp, 3, 130, byref(prm), bp, Tp, rep.words()) == -1
    assert viso.viso_tsdf_move(plain.h, dp, 3, 130, byref(prm), Tp, bp, rep.words()) == -1
    assert viso.viso_tsdf_move_gray(gmap.h, dp, ip, 3, 130, byref(prm), Tp, bp, rep.words()) == -1
    assert (_state(plain), _state(gmap)) == states and rep.as_dict() == dict.fromkeys(RT.REPORT, 7)
    # an overflowed map
    small = _map(False, {}, 10)
    big = scene((37, 333), False)[0]
    with pytest.raises(libviso_amd.VisoError, match="failed with -4"):
        small.fuse(big[0], prm, pose=big[1])
    with pytest.raises(libviso_amd.VisoError, match="failed with -4"):
        small.retract(big[0], prm, pose=big[1])
    with pytest.raises(libviso_amd.VisoError, match="failed with -4"):
        small.move(big[0], prm, big[1], POSES[2])
    # a dead handle
    h = plain.h
    for t in (plain, gmap, small):
        t.close()
    assert viso.viso_tsdf_retract(h, dp, 3, 130, byref(prm), Tp, rep.words()) == -1
    assert viso.viso_tsdf_move(h, dp, 3, 130, byref(prm), Tp, Tp, rep.words()) == -1
    assert rep.as_dict() == dict.fromkeys(RT.REPORT, 7)


@pytest.mark.parametrize("options", ["default", "both"])
@pytest.mark.parametrize("gray", [False, True])
def test_move(viso, gray, options):
    o = OPTIONS[options]
    A, B, C_ = scene((37, 333), gray)
    new = np.linalg.inv(hostmath.tr2mat([0.011, -0.019, 0.008, 0.33, -0.11, 1.43]))
    B_new = B[:-1] + (new,)
    e, st = fuse([A, B, C_], gray, o)
    want, wst = fuse([A, B_new, C_], gray, o)
    _, _, wrep, ok = retract(e, st, [B], gray, o)
    assert ok and not same(e, want)
    tsdf, fresh = _map(gray, o, _log2_for(max(len(e), len(want)))), _map(gray, o, _log2_for(max(len(e), len(want))))
    _fuse(tsdf, [A, B, C_])
    rep = tsdf.move(B[0], param(), B[-1], new, image=B[1] if gray else None)
    assert RT.same_report(rep, wrep)
    _check(tsdf, want, wst, (gray, options, "moved"))
    _fuse(fresh, [A, B_new, C_])
    _same_maps(tsdf, fresh, (gray, options))
    # a refused move changes nothing: B is not at its old pose any more
    _, _, wrep, ok = retract(want, wst, [B], gray, o)
    assert not ok
    before = _state(tsdf)
    with pytest.raises(libviso_amd.VisoError, match="failed with -1") as err:
        tsdf.move(B[0], param(), B[-1], POSES[2], image=B[1] if gray else None)
    assert RT.same_report(err.value.report, wrep) and _state(tsdf) == before
    tsdf.close(); fresh.close()


def _batch_with_maps(ctx, seq, **disp):
    nf, cap = seq["kp"].shape[0], seq["kp"].shape[2]
    b = libviso_amd.Batch(ctx, nf, cap)
    b.upload_images(seq["images"], seq["kp"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=3)
    b.set_disparity(**disp)
    return b


def test_resident_frames(viso):
    """The batch's calls on the resident maps and images: every frame retracted in one call, a sub-range moved in one call, a
    refused call, and a batch on another context."""
    seq = synth.make_subpixel_image_sequence(4, 4, n_kp=500, width=640, height=200)
    prm = seq["param"]
    ctx = libviso_amd.Context(0)
    b = _batch_with_maps(ctx, seq, num_disp=64)
    nf = b.nf
    b.run_images()
    T = np.array([np.linalg.inv(hostmath.tr2mat([0.0, 0.004 * t, 0.0, 0.02 * t, 0.0, -0.3 * t])) for t in range(nf)])
    T2 = T.copy()
    T2[1:3] = [np.linalg.inv(hostmath.tr2mat([0.001, 0.004 * t, 0.0, 0.02 * t + 0.01, 0.0, -0.3 * t - 0.02])) for t in (1, 2)]
    maps = [b.disparity(t) for t in range(nf)]
    want, st = CR.fuse([(maps[t], T[t]) for t in range(nf)], prm)
    moved, mst = CR.fuse([(maps[t], T2[t]) for t in range(nf)], prm)
    part, pst = CR.fuse([(maps[t], T[t]) for t in (1, 2)], prm)
    for s in (st, mst):
        assert s["n_out_of_range"] == 0 and s["n_dropped"] == 0 and s["n_points"] > 1000
    log2 = _log2_for(max(len(want), len(moved)))
    tsdf = libviso_amd.TsdfMap(ctx, capacity_log2=log2)
    b.fuse_tsdf(tsdf, T)
    _check(tsdf, want, st, "resident")
    # a sub-range moved: t0 > 0, t1 < n
    rep = b.move_tsdf(tsdf, T[1:3], T2[1:3], t0=1, t1=3)
    assert rep["n_points"] == pst["n_points"] and rep["n_updates"] == pst["n_updates"] and rep["n_missing"] == rep["n_underflow"] == 0
    _check(tsdf, moved, mst, "moved")
    # the old poses are not in the map any more: refused as a whole, nothing changes
    _, _, wrep, ok = RT.retract(moved, mst, [(maps[t], T[t]) for t in range(nf)], prm)
    assert not ok and wrep["n_points"] == st["n_points"]
    before = _state(tsdf)
    with pytest.raises(libviso_amd.VisoError, match="failed with -1") as err:
        b.retract_tsdf(tsdf, T)
    assert RT.same_report(err.value.report, wrep) and _state(tsdf) == before
    # every frame in one call: the empty map; and back
    rep = b.retract_tsdf(tsdf, T2)
    assert rep["n_freed"] == len(moved) and rep["n_updates"] == mst["n_updates"]
    assert len(tsdf.entries()) == 0 and tsdf.stats() == dict(n_points=0, n_updates=0, n_out_of_range=0, n_occupied=0, n_dropped=0)
    b.fuse_tsdf(tsdf, T)
    _check(tsdf, want, st, "fused again")
    # a gray map takes the resident left images: the same move against a map fused at the new poses
    gmap, gfresh = libviso_amd.TsdfMap(ctx, gray=True, capacity_log2=log2), libviso_amd.TsdfMap(ctx, gray=True, capacity_log2=log2)
    b.fuse_tsdf(gmap, T)
    b.move_tsdf(gmap, T[1:3], T2[1:3], t0=1, t1=3)
    b.fuse_tsdf(gfresh, T2)
    _same_maps(gmap, gfresh, "gray resident")
    assert same(gmap.entries(), moved)
    # a batch on another context
    other = libviso_amd.Context(0)
    far = libviso_amd.TsdfMap(other, capacity_log2=10)
    for call in (lambda: b.retract_tsdf(far, T), lambda: b.move_tsdf(far, T, T2)):
        with pytest.raises(libviso_amd.VisoError, match="failed with -1: .*share a context"):
            call()
    for v in (tsdf, gmap, gfresh, far):
        v.close()
    b.close(); ctx.close(); other.close()


def test_tool_reposes(viso, tmp_path):
    """fuse_map --repose writes the PLY of a plain run at the new poses, byte for byte, and says how many maps it moved."""
    frames = scene((37, 333), False)
    prm = param()
    d = tmp_path / "disp"
    d.mkdir()
    for i, (m, _) in enumerate(frames):
        fuse_map.write_disparity_png(str(d / ("%06d.png" % i)), np.where(m < 1, R.INVALID, m).astype(np.int16))
    old, new, calib = str(tmp_path / "poses.txt"), str(tmp_path / "new.txt"), str(tmp_path / "calib.txt")
    moved = [POSES[0], np.linalg.inv(hostmath.tr2mat([0.011, -0.019, 0.008, 0.33, -0.11, 1.43])), POSES[2]]
    fuse_map.write_poses(old, POSES)
    fuse_map.write_poses(new, moved)
    P0 = [prm.f, 0.0, prm.cu, 0.0, 0.0, prm.f, prm.cv, 0.0, 0.0, 0.0, 1.0, 0.0]
    P1 = list(P0)
    P1[3] = -prm.f * prm.base
    with open(calib, "w") as f:
        f.write("P0: " + " ".join("%.17g" % v for v in P0) + "\nP1: " + " ".join("%.17g" % v for v in P1) + "\n")
    outs = {}
    for tag, poses, args in (("old", old, []), ("new", new, []), ("reposed", old, ["--repose", new])):
        out = str(tmp_path / (tag + ".ply"))
        assert fuse_map.main([str(d), poses, calib, out, "--mesh", "--capacity-log2", "17"] + args) == 0
        outs[tag] = open(out, "rb").read()
    assert outs["reposed"] == outs["new"] != outs["old"]
    for bad in (["--window", "20"], ["--align"]):
        with pytest.raises(SystemExit):
            fuse_map.main([str(d), old, calib, str(tmp_path / "x.ply"), "--surface", "--repose", new] + bad)
