"""The frame-to-model alignment on the device (include/viso_hip.h, "TSDF align"; tsdf_linearize_kernel in
libviso_amd/csrc/tsdf_align.hip) against its numpy restatement (tests/align_ref.py): the sums of a linearise are integers, so
N.tobytes() and every counter are equal, and an alignment is followed step by step along the device's own trace, so that no bound
depends on two trajectories staying together.  Every table goes in through add_entries and the device's entries are asserted to
equal it.  Each case asserts its input condition on the restatement before the device is called."""
import math

import numpy as np
import pytest

import libviso_amd
from libviso_amd import hostmath, synth
from libviso_amd.abi import TSDF_ALIGNMENT_DTYPE, MatchParams, Param

import align_cases as AC
import align_ref as AR
import tsdf_ref as R
import tsdf_tables as TT

pytestmark = pytest.mark.gpu


def _loaded(entries, voxel, trunc=3, log2=16):
    tsdf = libviso_amd.TsdfMap(None, voxel=voxel, trunc_voxels=trunc, capacity_log2=log2)
    tsdf.add_entries(entries)
    got = tsdf.entries()
    assert got.dtype == entries.dtype and got.tobytes() == entries.tobytes()
    return tsdf


def _equal(got, want, tag):
    (N, c), (Nw, cw) = got, want
    assert N.dtype == Nw.dtype == np.int64 and N.shape == Nw.shape == (7, 7), tag
    assert c == cw, (tag, c, cw)
    assert N.tobytes() == Nw.tobytes(), (tag, np.argwhere(N != Nw)[:5].tolist())


@pytest.mark.parametrize("shape", [(3, 130), (1, 1), (37, 333)])
@pytest.mark.parametrize("voxel", [0.1, 0.2])
@pytest.mark.parametrize("trunc", [1, 3])
def test_linearize_equals_restatement(viso, shape, voxel, trunc):
    """(3, 130): runs that cross the wave boundaries at columns 63/64 and 127/128, and a short last wave.  The views see 35 degrees
    to each side where the fused ones saw 29, so the borders look past the model: some pixels are not used."""
    prm, e = AC.wide_param(shape), AC.model(voxel, trunc)
    cases = [("none", AC.FUSED[0], None), ("none, perturbed", AC.FUSED[0], AC.perturbed(np.eye(4))),
             ("rigid", AC.FUSED[1], AC.FUSED[1]), ("rigid, perturbed", AC.FUSED[1], AC.perturbed(AC.FUSED[1]))]
    wants = []
    for name, seen_from, pose in cases:
        m = AC.raycast(seen_from, shape, prm)
        want = AR.linearize(e, voxel, m, prm, pose)
        c = want[1]
        if m.size > 1:
            assert c["n_points"] == m.size and 2 * c["n_used"] >= c["n_points"] and c["n_used"] < c["n_points"], (name, c)
        else:
            assert c["n_points"] == 1 and c["n_used"] == 1, (name, c)    # one pixel cannot be both
        wants.append((m, want))
    assert len({w[0].tobytes() for _, w in wants}) == len(wants)          # every case differs
    tsdf = _loaded(e, voxel, trunc)
    for (name, _, pose), (m, want) in zip(cases, wants):
        _equal(tsdf.linearize(m, prm, pose), want, (shape, voxel, trunc, name))
    assert tsdf.entries().tobytes() == e.tobytes()
    tsdf.close()


@pytest.mark.parametrize("min_weight", [1, 2, 3])
def test_random_block_at_three_thresholds(viso, min_weight):
    """64^3 voxels at 70 % occupancy with weights 1..3.  The map looks into the block from before one of the cells that are usable
    at min_weight (at 3 there is one among a quarter of a million), with some pixels aimed into further ones."""
    e = AC.big_block()
    cells = AC.usable_cells(e, min_weight)
    pose = AC.before(cells[0], 0.2)
    m = AC.block_map()
    AC.aim(m, cells, 0.2, AC.BLOCK_PARAM, pose)
    want = AR.linearize(e, 0.2, m, AC.BLOCK_PARAM, pose, min_weight=min_weight)
    assert want[1]["n_missing"] > 0 and want[1]["n_used"] > 0, want[1]
    tsdf = _loaded(e, 0.2, log2=19)
    _equal(tsdf.linearize(m, AC.BLOCK_PARAM, pose, min_weight=min_weight), want, min_weight)
    print(f"min_weight {min_weight}: {len(cells)} usable cells, {want[1]}")
    tsdf.close()


def test_random_block_in_the_smallest_table(viso):
    """About 700 voxels in 2^10 slots: the eight lookups of a cell walk chains that wrap the table's end."""
    e = AC.small_block()
    m = AC.block_map()
    AC.aim(m, AC.usable_cells(e, 1), 0.2, AC.BLOCK_PARAM)
    want = AR.linearize(e, 0.2, m, AC.BLOCK_PARAM, None, min_weight=1)
    assert 650 < len(e) < 1024 and want[1]["n_missing"] > 0 and want[1]["n_used"] > 0, want[1]
    tsdf = _loaded(e, 0.2, log2=10)
    _equal(tsdf.linearize(m, AC.BLOCK_PARAM, None, min_weight=1), want, "2^10 slots")
    _equal(tsdf.linearize(m, AC.BLOCK_PARAM, AC.perturbed(np.eye(4)), min_weight=1),
           AR.linearize(e, 0.2, m, AC.BLOCK_PARAM, AC.perturbed(np.eye(4)), min_weight=1), "2^10 slots, perturbed")
    tsdf.close()


def test_gate_clip_key_range_and_large_weights(viso):
    # the gate: a random block's distances span the whole band
    e, m = AC.block(), AC.block_map()
    want = AR.linearize(e, 0.2, m, AC.BLOCK_PARAM, None, min_weight=1, gate_voxels=1.0)
    assert want[1]["n_gated"] > 0 and want[1]["n_used"] > 0, want[1]
    tsdf = _loaded(e, 0.2)
    _equal(tsdf.linearize(m, AC.BLOCK_PARAM, None, min_weight=1, gate_voxels=1.0), want, "gate")
    wide = AR.linearize(e, 0.2, m, AC.BLOCK_PARAM, None, min_weight=1, gate_voxels=3.0)
    assert wide[1]["n_gated"] < want[1]["n_gated"]
    _equal(tsdf.linearize(m, AC.BLOCK_PARAM, None, min_weight=1, gate_voxels=3.0), wide, "gate 3")
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        tsdf.linearize(m, AC.BLOCK_PARAM, None, gate_voxels=3.5)         # beyond the map's truncation
    tsdf.close()
    # the clip: points 0.27 m before a wall with f base = 388.8, w = f base / Z^2 > 4096
    shape = (3, 130)
    prm, e = AC.wide_param(shape), AC.model(0.1, 3)
    m = AC.raycast(AC.CLOSE, shape, prm)
    tsdf = _loaded(e, 0.1)
    want = AR.linearize(e, 0.1, m, prm, AC.CLOSE, gate_voxels=2.0)
    assert want[1]["n_clipped"] > 0, want[1]
    _equal(tsdf.linearize(m, prm, AC.CLOSE, gate_voxels=2.0), want, "clip")
    # a pose outside the key range: every point
    far = AC.view(tx=1e6)
    want = AR.linearize(e, 0.1, m, prm, far)
    assert want[1]["n_out_of_range"] == want[1]["n_points"] == m.size
    _equal(tsdf.linearize(m, prm, far), want, "key range")
    edge = AC.view(tx=float(1 << 20) * 0.1 - 0.1)                         # the cells of the range's last voxels along x
    want = AR.linearize(e, 0.1, m, prm, edge)
    assert 0 < want[1]["n_out_of_range"] < m.size, want[1]
    _equal(tsdf.linearize(m, prm, edge), want, "key range's edge")
    tsdf.close()
    # weights up to 2^31 and sums that are no multiple of the weight: a wall between the two layers of the slab
    c = TT.weights_and_means()
    prm = c[2]
    m = np.full(c[3], int(round(prm.f * prm.base / 2.2 * 16)), np.int16)
    want = AR.linearize(c[0], 0.2, m, prm, None, min_weight=1, gate_voxels=3.0)
    assert c[0]["weight"].max() == 1 << 31 and want[1]["n_used"] > 500 and want[1]["n_missing"] > 0, want[1]
    tsdf = _loaded(c[0], 0.2)
    _equal(tsdf.linearize(m, prm, None, min_weight=1, gate_voxels=3.0), want, "weights")
    rec, steps = tsdf.align(m, prm, None, trace=True, min_weight=1, gate_voxels=3.0)
    assert rec["status"] == -2 and len(steps) == 1 and rec["iters"] == 0 and rec["n_used"] == 0 and not rec["cov"].any()      # a single wall
    assert (rec["pose"] == np.eye(4)).all()
    tsdf.close()


def _follow(e, voxel, m, prm, rec, steps, p):
    """The device's trace against the restatement, step by step; returns the number of steps."""
    assert len(steps) >= 1
    status, iters = 2, 0
    for i, st in enumerate(steps):
        want = AR.linearize(e, voxel, m, prm, st["pose"], p["min_weight"], p["gate_voxels"])
        _equal(libviso_amd.tsdf_normal_matrix(st["normal"]), want, ("trace", i))
        assert (st["pose"][3] == (0, 0, 0, 1)).all()
        if i == len(steps) - 1:
            break
        code, xi, nxt = AR.step(want[0], want[1]["n_used"], st["pose"], p["min_pixels"])
        assert code == 0, (i, code)
        got = steps[i + 1]["pose"]
        assert np.abs(got[:3, :3] - nxt[:3, :3]).max() <= 1e-12 * np.abs(nxt[:3, :3]).max(), (i, np.abs(got - nxt).max())
        assert np.abs(got[:3, 3] - nxt[:3, 3]).max() <= 1e-12, (i, np.abs(got - nxt).max())
        iters = i + 1
        small = math.sqrt(sum(v * v for v in xi[3:])) <= p["eps_rot"] and math.sqrt(sum(v * v for v in xi[:3])) <= p["eps_trans"]
        assert small == (i == len(steps) - 2 and rec["status"] == 1), (i, xi)
        if small:
            status = 1
    last = AR.linearize(e, voxel, m, prm, steps[-1]["pose"], p["min_weight"], p["gate_voxels"])
    assert (rec["status"], rec["iters"], rec["n_used"]) == (status, iters, last[1]["n_used"])
    assert rec["pose"].tobytes() == steps[-1]["pose"].tobytes()
    code, _, _, C, L = AR.system(last[0], last[1]["n_used"], p["min_pixels"])
    assert code == 0 and abs(rec["cost"] - math.sqrt(C / last[1]["n_used"])) <= 1e-12 * rec["cost"]
    cov = rec["cov"]
    assert np.allclose(cov, cov.T, rtol=1e-9, atol=0) and (np.linalg.eigvalsh((cov + cov.T) / 2) > 0).all()
    H = last[0][:6, :6] / 65536.0
    assert np.allclose(cov @ H, np.eye(6) * C / (last[1]["n_used"] - 6), rtol=1e-6, atol=1e-9 * C / last[1]["n_used"])
    return iters


@pytest.mark.parametrize("voxel,gate,max_iters", [(0.1, 2.0, 10), (0.2, 1.0, 3)])
def test_align_follows_the_restatement_along_its_trace(viso, voxel, gate, max_iters):
    """The fourth view of the three-plane scene from a guess 0.45 degrees and 0.084 m off.  (0.2, 1.0, 3): max_iters ends it."""
    prm, e, m = AC.param(), AC.model(voxel, 3), AC.raycast(AC.TRUTH)
    p = dict(AR.DEFAULTS, gate_voxels=gate, max_iters=max_iters)
    tsdf = _loaded(e, voxel)
    rec, steps = tsdf.align(m, prm, AC.GUESS, trace=True, gate_voxels=gate, max_iters=max_iters)
    iters = _follow(e, voxel, m, prm, rec, steps, p)
    err, guess_err = AR.pose_error(rec["pose"], AC.TRUTH), AR.pose_error(AC.GUESS, AC.TRUTH)
    print(f"voxel {voxel}, gate {gate}: status {rec['status']}, {iters} steps, {rec['n_used']} pixels, cost {rec['cost']:.4f} px, "
          f"error {err[0]:.4f} degrees {err[1]:.5f} m from {guess_err[0]:.3f} degrees {guess_err[1]:.4f} m")
    assert rec["status"] == (1 if max_iters == 10 else 2) and err[0] < guess_err[0] and err[1] < guess_err[1]
    # without a trace: the same record; an align changes nothing in the map
    assert tsdf.align(m, prm, AC.GUESS, gate_voxels=gate, max_iters=max_iters).tobytes() == rec.tobytes()
    assert tsdf.entries().tobytes() == e.tobytes()
    # too few pixels: the guess comes back
    few = tsdf.align(m[:2, :90], prm, AC.GUESS, gate_voxels=gate)
    assert few["status"] == -1 and few["pose"].tobytes() == AC.GUESS.tobytes() and few["iters"] == 0 and few["cost"] == 0
    tsdf.close()


RES_SHAPE = (120, 400)


def _res_param():
    return Param.default(base=0.5371, f=360.0, cu=199.5, cv=59.5)


def test_resident_path_equals_single_calls_and_lifetime(viso):
    """The batch computes its maps itself, by block matching on textured stereo pairs of the three-plane scene (align_cases.stereo_pair):
    frames 0 and 1 from the first two fusing views, which make the model, frames 2..4 all from the fourth view, each aligned from a
    guess of its own."""
    prm = _res_param()
    seen = (AC.FUSED[0], AC.FUSED[1], AC.TRUTH, AC.TRUTH, AC.TRUTH)
    pairs = [AC.stereo_pair(T, RES_SHAPE, prm, seed=min(i, 2)) for i, T in enumerate(seen)]
    images = np.ascontiguousarray(np.stack([np.stack(p) for p in pairs]))
    nf = len(images)
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, nf, 64)
    b.upload_images_only(images)
    b.set_params(MatchParams.stereo(hostmath.F_from_P(synth.KITTI_P1, synth.KITTI_P2)), MatchParams.temporal(), prm)
    b.set_disparity(num_disp=64)
    tsdf = libviso_amd.TsdfMap(ctx, capacity_log2=18)
    guesses = np.stack([AC.perturbed(AC.TRUTH, 0.002 * (t + 1), 0.01 * (t + 1)) for t in range(3)])
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.align_tsdf(tsdf, guesses, t0=2, t1=5)                 # no run has computed the maps
    b.run_disparity()
    maps = [b.disparity(t) for t in range(nf)]
    assert all((m != R.INVALID).mean() > 0.5 for m in maps)
    b.fuse_tsdf(tsdf, np.stack(seen[:2]), t0=0, t1=2)           # the model
    model = tsdf.entries()
    par = dict(min_weight=1, gate_voxels=2.0, max_iters=8)
    # the input condition, on the restatement: every frame takes several steps and converges
    refs = [AR.align(model, 0.2, maps[2 + t], prm, guesses[t], **par)[0] for t in range(3)]
    assert all(r["status"] == 1 and r["iters"] >= 2 and r["n_used"] > 10000 for r in refs), [(r["status"], r["iters"], r["n_used"]) for r in refs]
    before = (b.disparities(), b.image(0, 0))
    single = np.stack([tsdf.align(maps[2 + t], prm, guesses[t], **par) for t in range(3)])
    assert single.dtype == TSDF_ALIGNMENT_DTYPE
    assert [(int(r["status"]), int(r["iters"]), int(r["n_used"])) for r in single] == [(r["status"], r["iters"], r["n_used"]) for r in refs]
    got = b.align_tsdf(tsdf, guesses, t0=2, t1=5, **par)
    assert got.dtype == TSDF_ALIGNMENT_DTYPE and got.tobytes() == single.tobytes()
    print("resident:", [(int(r["status"]), int(r["iters"]), int(r["n_used"])) for r in got])
    # a frame that finishes early (its guess looks away from the model: too few pixels at once) leaves its neighbours' records alone
    early = guesses.copy()
    early[1] = AC.view(ry=math.pi, tz=-50.0)
    got2 = b.align_tsdf(tsdf, early, t0=2, t1=5, **par)
    assert got2[1]["status"] == -1 and got2[1]["pose"].tobytes() == early[1].tobytes() and got2[1]["iters"] == 0
    assert got2[[0, 2]].tobytes() == single[[0, 2]].tobytes()
    assert b.align_tsdf(tsdf, guesses[2:], t0=4, t1=5, **par).tobytes() == single[2:].tobytes()
    # frames 1 and 2 are different maps (frames 2..4 are one map three times): a range that starts at 1 reads the maps it names
    g13 = np.stack([AC.perturbed(AC.FUSED[1], 0.002, 0.01), guesses[0]])
    mixed = np.stack([tsdf.align(maps[1 + t], prm, g13[t], **par) for t in range(2)])
    assert mixed[0]["status"] >= 1 and mixed[0].tobytes() != tsdf.align(maps[2], prm, g13[0], **par).tobytes()
    assert b.align_tsdf(tsdf, g13, t0=1, t1=3, **par).tobytes() == mixed.tobytes()
    # nothing else of the batch, and nothing of the map, has changed
    after = (b.disparities(), b.image(0, 0))
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert tsdf.entries().tobytes() == model.tobytes()
    # the refusals of the resident fuse
    for bad in (dict(t0=-1, t1=1, poses=guesses[:2]), dict(t0=0, t1=nf + 1, poses=np.tile(np.eye(4), (nf + 1, 1, 1))), dict(t0=2, t1=2, poses=guesses[:0])):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            b.align_tsdf(tsdf, bad["poses"], t0=bad["t0"], t1=bad["t1"])
    other = libviso_amd.TsdfMap(None, capacity_log2=12)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.align_tsdf(other, guesses, t0=2, t1=5)                # a map of another context
    other.close()
    nan = guesses.copy(); nan[1, 0, 0] = np.inf
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.align_tsdf(tsdf, nan, t0=2, t1=5)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.align_tsdf(tsdf, guesses, t0=2, t1=5, gate_voxels=4.0)
    # a map that outlives its context
    b.close(); ctx.close()
    for call in (lambda: tsdf.linearize(maps[0], prm), lambda: tsdf.align(maps[0], prm)):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            call()
    tsdf.close()
    assert tsdf.h is None


def test_overflow_refuses_and_clear_recovers(viso):
    prm = TT.param(f=2.0, cu=0.0, cv=0.0, base=1.0)
    wide = np.full((1, 2000), 16, np.int16)                     # one voxel of 0.5 m per pixel: 2000 for 1024 slots
    tsdf = libviso_amd.TsdfMap(None, voxel=0.5, trunc_voxels=1, min_disp16=1, capacity_log2=10)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.fuse(wide, prm)
    for call in (lambda: tsdf.linearize(wide, prm), lambda: tsdf.align(wide, prm)):
        with pytest.raises(libviso_amd.VisoError, match="-4"):
            call()
    tsdf.clear()
    e = AC.small_block()
    tsdf.close()
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=10)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.add_entries(np.concatenate([e, AC.block()]))       # more than 1024 voxels
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.linearize(AC.block_map(), AC.BLOCK_PARAM)
    tsdf.clear()
    tsdf.add_entries(e)
    m = AC.block_map()
    AC.aim(m, AC.usable_cells(e, 1), 0.2, AC.BLOCK_PARAM)
    _equal(tsdf.linearize(m, AC.BLOCK_PARAM, None, min_weight=1), AR.linearize(e, 0.2, m, AC.BLOCK_PARAM, None, min_weight=1), "after clear")
    tsdf.close()


def test_full_frame_once(viso):
    shape = (376, 1241)
    prm, e = AC.param(shape), AC.model(0.1, 3)
    m = AC.raycast(AC.TRUTH, shape, prm)
    pose = AC.perturbed(AC.TRUTH)
    want = AR.linearize(e, 0.1, m, prm, pose, gate_voxels=2.0)
    assert want[1]["n_points"] == m.size and 2 * want[1]["n_used"] >= m.size, want[1]
    tsdf = _loaded(e, 0.1)
    _equal(tsdf.linearize(m, prm, pose, gate_voxels=2.0), want, "full frame")
    print(f"full frame: {want[1]}, largest sum 2^{math.log2(float(np.abs(want[0]).max())):.1f}")
    tsdf.close()
