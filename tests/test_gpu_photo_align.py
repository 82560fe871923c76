"""The photometric frame-to-model alignment on the device (include/viso_hip.h, "TSDF photometric align";
tsdf_gray_linearize_kernel in libviso_amd/csrc/tsdf_align.hip) against its numpy restatement (tests/photo_align_ref.py): the sums
of a linearise are integers, so N.tobytes(), p and the nine counters are equal, and an alignment is followed step by step along the
device's own trace.  Every table goes in through add_entries and the device's entries are asserted to equal it before and after.
Each case asserts its input condition on the restatement before the device is called."""
import ctypes as C
import math

import numpy as np
import pytest

import libviso_amd
from libviso_amd import hostmath, synth
from libviso_amd.abi import (TSDF_ALIGN_GRAY_STEP_DTYPE, TSDF_ALIGNMENT_DTYPE, TSDF_ALIGNMENT_GRAY_DTYPE, TSDF_NORMAL_GRAY_DTYPE, MatchParams,
                             Param)

import align_cases as AC
import align_ref as AR
import gray_ref as GR
import photo_align_cases as PC
import photo_align_ref as PR
import tsdf_ref as R
import tsdf_tables as TT

pytestmark = pytest.mark.gpu


def _loaded(entries, voxel, trunc=3, log2=16, ctx=None):
    tsdf = libviso_amd.TsdfMap(ctx, gray=True, voxel=voxel, trunc_voxels=trunc, capacity_log2=log2)
    tsdf.add_entries(entries)
    _unchanged(tsdf, entries)
    return tsdf


def _unchanged(tsdf, entries):
    got = tsdf.entries(gray=True)
    assert got.dtype == entries.dtype and got.tobytes() == entries.tobytes()


def _only_the_guess(rec, guess, status):
    """A failed alignment's record: the guess, the status, and every other number zero."""
    assert rec["status"] == status and rec["pose"].tobytes() == np.asarray(guess).tobytes()
    assert all(not np.any(rec[k]) for k in rec.dtype.names if k not in ("pose", "status")), rec


def _equal(got, want, tag):
    (N, p, c), (Nw, pw, cw) = got, want
    assert N.dtype == Nw.dtype == np.int64 and N.shape == Nw.shape == (7, 7), tag
    assert c == cw and len(c) == 9, (tag, c, cw)
    assert p == pw, (tag, p, pw)
    assert N.tobytes() == Nw.tobytes(), (tag, np.argwhere(N != Nw)[:5].tolist())


@pytest.mark.parametrize("shape", [(3, 130), (1, 1), (37, 333)])
@pytest.mark.parametrize("voxel", [0.1, 0.2])
def test_linearize_equals_restatement(viso, shape, voxel):
    """(3, 130): runs that cross the wave boundaries at columns 63/64 and 127/128, and a short last wave.  The views see 35 degrees
    to each side where the fused ones saw 29: some pixels are not used."""
    prm, e = AC.wide_param(shape), PC.model("room", voxel)
    cases = [("none", AC.FUSED[0], None), ("none, perturbed", AC.FUSED[0], AC.perturbed(np.eye(4))),
             ("rigid", AC.FUSED[1], AC.FUSED[1]), ("rigid, perturbed", AC.FUSED[1], AC.perturbed(AC.FUSED[1]))]
    wants = []
    for name, seen_from, pose in cases:
        m, g = PC.raycast(seen_from, "room", shape, prm)
        want = PR.linearize(e, voxel, m, g, prm, pose)
        c = want[2]
        if m.size > 1:
            assert c["n_points"] == m.size and 2 * c["n_used"] >= c["n_points"] and c["n_used"] < c["n_points"], (name, c)
            assert c["n_photo_used"] == c["n_used"] and want[1] > 0, (name, c)
        else:
            assert c["n_points"] == 1 and c["n_used"] == c["n_photo_used"] == 1, (name, c)
        wants.append((m, g, want))
    assert len({w[0].tobytes() for _, _, w in wants}) == len(wants)       # every case differs
    tsdf = _loaded(e, voxel)
    for (name, _, pose), (m, g, want) in zip(cases, wants):
        _equal(tsdf.linearize(m, prm, pose, image=g), want, (shape, voxel, name))
    _unchanged(tsdf, e)
    tsdf.close()


@pytest.mark.parametrize("min_weight", [1, 2, 3])
def test_random_block_at_three_thresholds(viso, min_weight):
    """64^3 voxels at 70 % occupancy with weights 1..3 and random sums of intensities, under a random image."""
    e = PC.random_gray(AC.big_block())
    cells = AC.usable_cells(e, min_weight)
    pose = AC.before(cells[0], 0.2)
    m = AC.block_map()
    AC.aim(m, cells, 0.2, AC.BLOCK_PARAM, pose)
    g = np.random.default_rng(12).integers(0, 256, m.shape).astype(np.uint8)
    want = PR.linearize(e, 0.2, m, g, AC.BLOCK_PARAM, pose, min_weight=min_weight, photo_gate=100.0)
    c = want[2]
    assert c["n_missing"] > 0 and c["n_used"] > 0 and c["n_photo_used"] > 0 and (min_weight > 1 or c["n_photo_gated"] > 0), c
    tsdf = _loaded(e, 0.2, log2=19)
    _equal(tsdf.linearize(m, AC.BLOCK_PARAM, pose, image=g, min_weight=min_weight, photo_gate=100.0), want, min_weight)
    print(f"min_weight {min_weight}: {len(cells)} usable cells, {c}")
    tsdf.close()


def test_one_run_gate_and_clip(viso):
    # a full wave as one run: 64 lanes take their eight voxels' three words from lane 0
    e, voxel, m, g, prm = PC.one_run_case()
    want = PR.linearize(e, voxel, m, g, prm, None)
    assert want[2]["n_photo_used"] == want[2]["n_used"] == 128 and want[1] > 0, want[2]
    tsdf = _loaded(e, voxel, log2=10)
    _equal(tsdf.linearize(m, prm, None, image=g), want, "one run")
    tsdf.close()
    # P5: a table built by hand, at the default lambda
    e, voxel, m, g, prm = PC.clip_case()
    want = PR.linearize(e, voxel, m, g, prm, None)
    assert want[2]["n_photo_clipped"] > 100 and want[2]["n_photo_used"] > 100 and want[2]["n_clipped"] == 0, want[2]
    tsdf = _loaded(e, voxel, log2=10)
    _equal(tsdf.linearize(m, prm, None, image=g), want, "clip")
    tsdf.close()
    # P3: a gate that ends some rows and not all; the geometric rows stay
    e, (m, g), prm = PC.model("wall", 0.1), PC.frame("wall"), AC.param()
    tsdf = _loaded(e, 0.1)
    want = PR.linearize(e, 0.1, m, g, prm, AC.GUESS, gate_voxels=2.0, photo_gate=10.0)
    c = want[2]
    assert c["n_photo_gated"] > 1000 and c["n_photo_used"] > 1000 and c["n_photo_gated"] + c["n_photo_used"] == c["n_used"], c
    _equal(tsdf.linearize(m, prm, AC.GUESS, image=g, gate_voxels=2.0, photo_gate=10.0), want, "photo gate")
    # lambda = 0: the plain linearise's sums and counters, byte for byte, on the same map
    N0, p0, c0 = tsdf.linearize(m, prm, AC.GUESS, image=g, gate_voxels=2.0, photo_weight=0.0)
    Np, cp = tsdf.linearize(m, prm, AC.GUESS, gate_voxels=2.0)
    assert N0.tobytes() == Np.tobytes() and p0 == 0 and {k: c0[k] for k in AR.COUNTERS} == cp and c0["n_photo_used"] == cp["n_used"] > 0
    # the raw struct: its leading 272 bytes are the plain call's
    L, p, pp = tsdf.L, libviso_amd.tsdf_align_gray_params(gate_voxels=2.0, photo_weight=0.0), libviso_amd.tsdf_align_params(gate_voxels=2.0)
    out_g, out_p = np.zeros(1, TSDF_NORMAL_GRAY_DTYPE), np.zeros(1, libviso_amd.abi.TSDF_NORMAL_DTYPE)
    T = np.ascontiguousarray(AC.GUESS)
    mp, ip, Tp = m.ctypes.data_as(C.POINTER(C.c_int16)), g.ctypes.data_as(C.POINTER(C.c_uint8)), T.ctypes.data_as(C.POINTER(C.c_double))
    assert L.viso_tsdf_linearize_gray(tsdf.h, C.byref(p), mp, ip, m.shape[0], m.shape[1], C.byref(prm), Tp, out_g.ctypes.data) == 1
    assert L.viso_tsdf_linearize(tsdf.h, C.byref(pp), mp, m.shape[0], m.shape[1], C.byref(prm), Tp, out_p.ctypes.data) == 1
    assert out_g.tobytes()[:272] == out_p.tobytes()
    _unchanged(tsdf, e)
    tsdf.close()


def _follow(e, voxel, m, g, prm, rec, steps, p, photo):
    """The device's trace against the restatement, step by step; returns the number of steps."""
    assert len(steps) >= 1 and steps.dtype == TSDF_ALIGN_GRAY_STEP_DTYPE

    def lin(pose):
        return PR.linearize(e, voxel, m, g, prm, pose, p["min_weight"], p["gate_voxels"], photo["photo_weight"], photo["photo_gate"])

    status, iters = 2, 0
    for i, st in enumerate(steps):
        want = lin(st["pose"])
        _equal(libviso_amd.tsdf_normal_gray_matrix(st["normal"]), want, ("trace", i))
        assert (st["pose"][3] == (0, 0, 0, 1)).all()
        if i == len(steps) - 1:
            break
        code, xi, nxt = AR.step(want[0], want[2]["n_used"], st["pose"], p["min_pixels"])
        assert code == 0, (i, code)
        got = steps[i + 1]["pose"]
        assert np.abs(got[:3, :3] - nxt[:3, :3]).max() <= 1e-12 * np.abs(nxt[:3, :3]).max(), (i, np.abs(got - nxt).max())
        assert np.abs(got[:3, 3] - nxt[:3, 3]).max() <= 1e-12, (i, np.abs(got - nxt).max())
        iters = i + 1
        small = math.sqrt(sum(v * v for v in xi[3:])) <= p["eps_rot"] and math.sqrt(sum(v * v for v in xi[:3])) <= p["eps_trans"]
        assert small == (i == len(steps) - 2 and rec["status"] == 1), (i, xi)
        if small:
            status = 1
    N, pp, c = lin(steps[-1]["pose"])
    want = PR.record((steps[-1]["pose"], N, dict(c, p=pp)), status, iters, photo["photo_weight"])
    assert (rec["status"], rec["iters"], rec["n_used"], rec["n_photo_used"]) == (status, iters, c["n_used"], c["n_photo_used"])
    assert rec["pose"].tobytes() == steps[-1]["pose"].tobytes()
    for k in ("cost", "cost_geo", "cost_photo"):
        assert abs(rec[k] - want[k]) <= 1e-12 * want[k], (k, rec[k], want[k])
    assert np.abs(rec["cov"] - want["cov"]).max() <= 1e-9 * np.abs(want["cov"]).max()
    cov = rec["cov"]
    assert np.allclose(cov, cov.T, rtol=1e-9, atol=0) and (np.linalg.eigvalsh((cov + cov.T) / 2) > 0).all()
    return iters


@pytest.mark.parametrize("voxel,gate,max_iters", [(0.1, 2.0, 10), (0.2, 1.0, 10), (0.2, 1.0, 2)])
def test_align_on_the_wall_follows_the_restatement_along_its_trace(viso, voxel, gate, max_iters):
    """The textured wall from a guess 0.45 degrees and 0.084 m off: the plain alignment on the same device map does not hold it,
    the photometric one ends at the truth.  (0.2, 1.0, 2): max_iters ends it."""
    prm, e, (m, g) = AC.param(), PC.model("wall", voxel), PC.frame("wall")
    p, photo = dict(AR.DEFAULTS, gate_voxels=gate, max_iters=max_iters), PR.PHOTO_DEFAULTS
    tsdf = _loaded(e, voxel)
    rec, steps = tsdf.align(m, prm, AC.GUESS, trace=True, image=g, gate_voxels=gate, max_iters=max_iters)
    assert rec.dtype == TSDF_ALIGNMENT_GRAY_DTYPE
    iters = _follow(e, voxel, m, g, prm, rec, steps, p, photo)
    err, guess_err = AR.pose_error(rec["pose"], AC.TRUTH), AR.pose_error(AC.GUESS, AC.TRUTH)
    plain = tsdf.align(m, prm, AC.GUESS, gate_voxels=gate)
    plain_err = AR.pose_error(plain["pose"], AC.TRUTH)
    print(f"voxel {voxel}, gate {gate}: status {rec['status']}, {iters} steps, {rec['n_photo_used']} of {rec['n_used']} rows, cost "
          f"{rec['cost_geo']:.4f} px {rec['cost_photo']:.3f} gray levels, error {err[0]:.5f} degrees {err[1]:.6f} m; plain: status "
          f"{plain['status']}, {plain_err[0]:.5f} degrees {plain_err[1]:.6f} m; guess {guess_err[0]:.3f} degrees {guess_err[1]:.4f} m")
    assert plain.dtype == TSDF_ALIGNMENT_DTYPE and plain["status"] > 0
    if max_iters == 10:
        measured = {0.1: (0.00181, 0.000648), 0.2: (0.00923, 0.000665)}[voxel]            # tests/test_photo_align_cpu.py's MEASURED
        assert plain_err[1] > 0.5 * guess_err[1] if voxel == 0.1 else plain_err[0] > guess_err[0]
        assert rec["status"] == 1 and iters <= 6 and err[0] <= 2 * measured[0] and err[1] <= 2 * measured[1] and err[1] < 0.1 * plain_err[1]
    else:
        assert rec["status"] == 2 and iters == 2 and err[1] < guess_err[1]
    # without a trace: the same record; the calls change nothing in the map
    assert tsdf.align(m, prm, AC.GUESS, image=g, gate_voxels=gate, max_iters=max_iters).tobytes() == rec.tobytes()
    _unchanged(tsdf, e)
    # too few pixels: the guess comes back, everything else zero
    few = tsdf.align(m[:2, :90], prm, AC.GUESS, image=np.ascontiguousarray(g[:2, :90]), gate_voxels=gate)
    _only_the_guess(few, AC.GUESS, -1)
    tsdf.close()


RES_SHAPE = (120, 400)


def test_resident_path_equals_single_calls_and_lifetime(viso):
    """The batch computes its maps itself, by block matching on textured stereo pairs of the three-plane scene
    (align_cases.stereo_pair), and fuses frames 0 and 1 with their left images into a gray map; frames 2..4, all from the fourth
    view, are aligned with their resident left images, each from a guess of its own."""
    prm = Param.default(base=0.5371, f=360.0, cu=199.5, cv=59.5)
    seen = (AC.FUSED[0], AC.FUSED[1], AC.TRUTH, AC.TRUTH, AC.TRUTH)
    pairs = [AC.stereo_pair(T, RES_SHAPE, prm, seed=min(i, 2)) for i, T in enumerate(seen)]
    images = np.ascontiguousarray(np.stack([np.stack(p) for p in pairs]))
    nf = len(images)
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, nf, 64)
    b.upload_images_only(images)
    b.set_params(MatchParams.stereo(hostmath.F_from_P(synth.KITTI_P1, synth.KITTI_P2)), MatchParams.temporal(), prm)
    b.set_disparity(num_disp=64)
    tsdf = libviso_amd.TsdfMap(ctx, gray=True, capacity_log2=18)
    guesses = np.stack([AC.perturbed(AC.TRUTH, 0.002 * (t + 1), 0.01 * (t + 1)) for t in range(3)])
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.align_tsdf(tsdf, guesses, t0=2, t1=5, photo=True)     # no run has computed the maps
    b.run_disparity()
    maps = [b.disparity(t) for t in range(nf)]
    lefts = [b.image(t, 0) for t in range(nf)]
    assert all((m != R.INVALID).mean() > 0.5 for m in maps) and all(np.array_equal(lefts[t], images[t, 0]) for t in range(nf))
    b.fuse_tsdf(tsdf, np.stack(seen[:2]), t0=0, t1=2)           # the model, with the resident left images
    model = tsdf.entries(gray=True)
    assert model.tobytes() == GR.fuse([(maps[t], lefts[t], seen[t]) for t in range(2)], prm)[0].tobytes()
    par = dict(min_weight=1, gate_voxels=2.0, max_iters=8)
    # the input condition, on the restatement: every frame takes at least two steps
    refs = [PR.align(model, 0.2, maps[2 + t], lefts[2 + t], prm, guesses[t], **par)[0] for t in range(3)]
    assert all(r["status"] > 0 and r["iters"] >= 2 and r["n_photo_used"] > 10000 for r in refs), [(r["status"], r["iters"], r["n_used"]) for r in refs]
    before = (b.disparities(), b.image(0, 0), b.image(2, 0), b.image(2, 1))
    single = np.stack([tsdf.align(maps[2 + t], prm, guesses[t], image=lefts[2 + t], **par) for t in range(3)])
    assert single.dtype == TSDF_ALIGNMENT_GRAY_DTYPE
    assert ([(int(r["status"]), int(r["iters"]), int(r["n_used"]), int(r["n_photo_used"])) for r in single]
            == [(r["status"], r["iters"], r["n_used"], r["n_photo_used"]) for r in refs])
    got = b.align_tsdf(tsdf, guesses, t0=2, t1=5, photo=True, **par)
    assert got.dtype == TSDF_ALIGNMENT_GRAY_DTYPE and got.tobytes() == single.tobytes()
    print("resident:", [(int(r["status"]), int(r["iters"]), int(r["n_used"]), float(r["cost_geo"]), float(r["cost_photo"])) for r in got])
    # the plain call on the gray map is the plain call: the existing record type, no photometric fields
    plain = b.align_tsdf(tsdf, guesses, t0=2, t1=5, **par)
    assert plain.dtype == TSDF_ALIGNMENT_DTYPE
    assert plain.tobytes() == np.stack([tsdf.align(maps[2 + t], prm, guesses[t], **par) for t in range(3)]).tobytes()
    # a frame that finishes early (its guess looks away from the model) leaves its neighbours' records alone
    early = guesses.copy()
    early[1] = AC.view(ry=math.pi, tz=-50.0)
    got2 = b.align_tsdf(tsdf, early, t0=2, t1=5, photo=True, **par)
    _only_the_guess(got2[1], early[1], -1)
    assert got2[[0, 2]].tobytes() == single[[0, 2]].tobytes()
    assert b.align_tsdf(tsdf, guesses[2:], t0=4, t1=5, photo=True, **par).tobytes() == single[2:].tobytes()
    # frames 1 and 2 are different maps and images (frames 2..4 are one pair three times): a range that starts at 1 reads what it names
    g13 = np.stack([AC.perturbed(AC.FUSED[1], 0.002, 0.01), guesses[0]])
    mixed = np.stack([tsdf.align(maps[1 + t], prm, g13[t], image=lefts[1 + t], **par) for t in range(2)])
    assert mixed[0]["status"] >= 1 and mixed[0].tobytes() != tsdf.align(maps[2], prm, g13[0], image=lefts[2], **par).tobytes()
    assert mixed[0].tobytes() != tsdf.align(maps[1], prm, g13[0], image=lefts[2], **par).tobytes()   # the image matters as well
    assert b.align_tsdf(tsdf, g13, t0=1, t1=3, photo=True, **par).tobytes() == mixed.tobytes()
    # nothing else of the batch, and nothing of the map, has changed
    after = (b.disparities(), b.image(0, 0), b.image(2, 0), b.image(2, 1))
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert tsdf.entries(gray=True).tobytes() == model.tobytes()
    # the refusals of the resident fuse
    for bad in (dict(t0=-1, t1=1, poses=guesses[:2]), dict(t0=0, t1=nf + 1, poses=np.tile(np.eye(4), (nf + 1, 1, 1))), dict(t0=2, t1=2, poses=guesses[:0])):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b.align_tsdf(tsdf, bad["poses"], t0=bad["t0"], t1=bad["t1"], photo=True)
    other = libviso_amd.TsdfMap(None, gray=True, capacity_log2=12)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.align_tsdf(other, guesses, t0=2, t1=5, photo=True)    # a map of another context
    other.close()
    flat = libviso_amd.TsdfMap(ctx, capacity_log2=12)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.align_tsdf(flat, guesses, t0=2, t1=5, photo=True)     # a plain map
    flat.close()
    nan = guesses.copy(); nan[1, 0, 0] = np.inf
    for kw in (dict(poses=nan), dict(gate_voxels=4.0), dict(photo_weight=-1.0), dict(photo_gate=0.0)):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b.align_tsdf(tsdf, kw.pop("poses", guesses), t0=2, t1=5, photo=True, **kw)
    # a map that outlives its context
    b.close(); ctx.close()
    for call in (lambda: tsdf.linearize(maps[0], prm, image=lefts[0]), lambda: tsdf.align(maps[0], prm, image=lefts[0])):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            call()
    tsdf.close()
    assert tsdf.h is None


def test_kinds_do_not_mix(viso):
    """The photometric calls on a plain map, and a null image on a gray one: VISO_ERR_ARG, both tables untouched.  The plain calls
    on a gray map are the plain calls."""
    e, (m, g), prm = PC.model("wall", 0.2), PC.frame("wall"), AC.param()
    gray, plain = _loaded(e, 0.2), libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=16)
    pe = GR.plain(e)
    plain.add_entries(pe)
    gst, pst = gray.stats(), plain.stats()
    L = gray.L
    p = libviso_amd.tsdf_align_gray_params()
    out, rec = np.zeros(1, TSDF_NORMAL_GRAY_DTYPE), np.zeros(1, TSDF_ALIGNMENT_GRAY_DTYPE)
    mp, ip = m.ctypes.data_as(C.POINTER(C.c_int16)), g.ctypes.data_as(C.POINTER(C.c_uint8))
    rows, cols = m.shape
    assert L.viso_tsdf_linearize_gray(plain.h, C.byref(p), mp, ip, rows, cols, C.byref(prm), None, out.ctypes.data) == -1
    assert b"viso_tsdf_linearize_gray" in L.viso_last_error() and b"no intensity" in L.viso_last_error()
    assert L.viso_tsdf_align_gray(plain.h, C.byref(p), mp, ip, rows, cols, C.byref(prm), None, rec.ctypes.data, None, 0) == -1
    assert b"viso_tsdf_align_gray" in L.viso_last_error() and b"no intensity" in L.viso_last_error()
    assert L.viso_tsdf_linearize_gray(gray.h, C.byref(p), mp, None, rows, cols, C.byref(prm), None, out.ctypes.data) == -1
    assert L.viso_tsdf_align_gray(gray.h, C.byref(p), mp, None, rows, cols, C.byref(prm), None, rec.ctypes.data, None, 0) == -1
    assert not out.tobytes().strip(b"\0") and not rec.tobytes().strip(b"\0")
    for t in (plain,):
        with pytest.raises(ValueError):
            t.linearize(m, prm, image=g)
        with pytest.raises(ValueError):
            t.align(m, prm, image=g)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        gray.linearize(m, prm, image=g, gate_voxels=3.5)         # beyond the map's truncation
    # the plain calls take either kind and give the same
    Ng, cg = gray.linearize(m, prm, AC.GUESS)
    Np, cp = plain.linearize(m, prm, AC.GUESS)
    assert Ng.tobytes() == Np.tobytes() and cg == cp and cg["n_used"] > 10000
    assert gray.align(m, prm, AC.GUESS).tobytes() == plain.align(m, prm, AC.GUESS).tobytes()
    _unchanged(gray, e)
    assert plain.entries().tobytes() == pe.tobytes() and gray.stats() == gst and plain.stats() == pst
    gray.close(); plain.close()
    assert L.viso_tsdf_linearize_gray(gray.h, C.byref(p), mp, ip, rows, cols, C.byref(prm), None, out.ctypes.data) == -1


def test_overflow_refuses_and_clear_recovers(viso):
    prm = TT.param(f=2.0, cu=0.0, cv=0.0, base=1.0)
    wide, img = np.full((1, 2000), 16, np.int16), np.full((1, 2000), 7, np.uint8)   # one voxel of 0.5 m per pixel: 2000 for 1024 slots
    tsdf = libviso_amd.TsdfMap(None, gray=True, voxel=0.5, trunc_voxels=1, min_disp16=1, capacity_log2=10)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.fuse(wide, prm, image=img)
    for call in (lambda: tsdf.linearize(wide, prm, image=img), lambda: tsdf.align(wide, prm, image=img)):
        with pytest.raises(libviso_amd.VisoError, match="-4"):
            call()
    tsdf.close()
    e, voxel, m, g, prm = PC.one_run_case()
    tsdf = libviso_amd.TsdfMap(None, gray=True, voxel=voxel, capacity_log2=10)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.add_entries(np.concatenate([e, PC.clip_case()[0], PC.random_gray(AC.small_block())]))   # more than 1024 voxels
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.linearize(m, prm, image=g)
    tsdf.clear()
    tsdf.add_entries(e)
    _equal(tsdf.linearize(m, prm, None, image=g), PR.linearize(e, voxel, m, g, prm, None), "after clear")
    tsdf.close()


def test_full_frame_once(viso):
    shape = (376, 1241)
    prm, e = AC.param(shape), PC.model("room", 0.1)
    m, g = PC.raycast(AC.TRUTH, "room", shape, prm)
    pose = AC.perturbed(AC.TRUTH)
    want = PR.linearize(e, 0.1, m, g, prm, pose, gate_voxels=2.0)
    c = want[2]
    assert c["n_points"] == m.size and 2 * c["n_used"] >= m.size and c["n_photo_used"] == c["n_used"], c
    tsdf = _loaded(e, 0.1)
    _equal(tsdf.linearize(m, prm, pose, image=g, gate_voxels=2.0), want, "full frame")
    print(f"full frame: {c}, p 2^{math.log2(float(want[1])):.1f}, largest sum 2^{math.log2(float(np.abs(want[0]).max())):.1f}")
    tsdf.close()
