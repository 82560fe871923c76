"""The ray casting and the crossings of the TSDF map on the device (tsdf_render_kernel, tsdf_crossings_kernel in
libviso_amd/csrc/tsdf.hip) on the hand-built tables of tests/tsdf_tables.py, byte for byte against the numpy restatements
(tests/render_ref.py, tests/tsdf_ref.py).  tests/test_gpu_render.py feeds the ray casting fused scenes only; there no sample is
outside the key range, no hit has an invalid value, no ray starts inside the surface, and the lanes of a wave do the same thing at
the same sample.  Here every table goes in through add_entries, the device's entries are asserted to equal it, and:

  random blocks   every lane of a wave at a different place in the rule, at min_weight 1, 2, 3; once from a table of 2^10 slots
  too_big, too_small, behind   a hit whose value is invalid ends the march: INVALID though a valid surface lies behind
  gap_in, gap_out, gap_beside  samples outside the key range, before the surface, behind it, and a ray of nothing else
  weights_and_means            wa > wb and wa < wb, weights of 2^31, sums at the ends of the band and no multiple of the weight

The key range is a convex box and a ray is a straight line, so the gaps of a ray can only lead or trail it: "a gap empties
previous" (step 4 of the rule) has no observable effect for a finite pose, and no case aims at it.

Input condition, asserted on the restatement before any device call: the trace count (render_ref.EVENTS) the case exists for is
> 0, by the loop restatement, which must agree with the vectorised one; for the sweeps over the random blocks, whose traces
tests/test_render_cpu.py asserts, at least 5 % of every view's pixels are valid and at least 5 % invalid (a block of 70 %
occupancy cannot be half valid at min_weight 3).  The device is compared with the vectorised restatement."""
import numpy as np
import pytest

import libviso_amd

import render_ref as RR
import tsdf_ref as R
import tsdf_tables as TT

pytestmark = pytest.mark.gpu

INV = R.INVALID


def _equal(got, want, tag):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, tag
        assert g.tobytes() == w.tobytes(), (tag, int((g != w).sum()), np.argwhere(g != w)[:5].tolist())


def _loaded(entries, voxel, log2=13):
    tsdf = libviso_amd.TsdfMap(None, voxel=voxel, capacity_log2=log2)
    tsdf.add_entries(entries)
    got = tsdf.entries()
    assert got.dtype == entries.dtype and got.tobytes() == entries.tobytes()
    return tsdf


def _render(tsdf, case):
    _, _, prm, shape, pose, max_depth, mw = case
    return tsdf.render(prm, shape, pose, max_depth=max_depth, min_weight=mw, weights=True)


def _want_traced(name):
    """The case, what the vectorised restatement gives for it, and its trace; the loop restatement agrees and the event is there."""
    fn, event = TT.SMALL_CASES[name]
    case = fn()
    want = RR.render(*case)
    d, w, trace = TT.events(case)
    assert d.tobytes() == want[0].tobytes() and w.tobytes() == want[1].tobytes(), name
    assert ((want[0] == INV) == (want[1] == 0)).all()
    assert trace[event] > 0, (name, dict(trace))
    print(f"{name}: {len(case[0])} voxels, {(want[0] != INV).mean():.3f} valid, {dict(trace)}")
    return case, want, trace


def _share(d, tag):
    valid = float((d != INV).mean())
    assert 0.05 <= valid <= 0.95, (tag, valid)
    return valid


@pytest.mark.parametrize("name", list(TT.BLOCKS))
def test_random_blocks(viso, name):
    """far: the camera a voxel before a 12^3 block, from three poses.  inside: the camera in the first layer of a 10^3 block, so
    that rays start in a negative voxel.  Both 70 % / 60 % occupied with weights 1..3."""
    sweep = TT.block_sweep(name)
    wants = []
    for pose, mw, case in sweep:
        want = RR.render(*case)
        assert ((want[0] == INV) == (want[1] == 0)).all() and (want[1][want[0] != INV] >= mw).all()
        wants.append((want, _share(want[0], (name, pose, mw))))
    assert len({w[0].tobytes() for w, _ in wants}) == len(wants)          # every view differs
    tsdf = _loaded(sweep[0][2][0], 0.2)
    for (pose, mw, case), (want, valid) in zip(sweep, wants):
        _equal(_render(tsdf, case), want, (name, pose, mw, valid))
    print(f"{name}: {len(sweep[0][2][0])} voxels, valid shares {[round(v, 3) for _, v in wants]}")
    tsdf.close()


def test_random_block_in_the_smallest_table(viso):
    """About 700 voxels in 2^10 slots: the march's lookups walk chains of tens of slots that wrap the table's end."""
    cases = [TT.chains_view(mw) for mw in TT.BLOCK_MIN_WEIGHTS]
    assert 680 <= len(cases[0][0]) <= 729
    wants = [RR.render(*c) for c in cases]
    for mw, w in zip(TT.BLOCK_MIN_WEIGHTS, wants):
        _share(w[0], ("chains", mw))
    tsdf = _loaded(cases[0][0], 0.2, log2=10)
    for mw, c, w in zip(TT.BLOCK_MIN_WEIGHTS, cases, wants):
        _equal(_render(tsdf, c), w, ("chains", mw))
    tsdf.close()


def test_a_hit_that_is_too_near_ends_the_march(viso):
    """v >= 32768 at the near slab: INVALID at every pixel, though the far slab alone gives 3034 at every pixel."""
    case, want, trace = _want_traced("too_big")
    alone, want_alone, trace_alone = _want_traced("too_big_alone")
    n = want[0].size
    assert n == 45 and trace["hit_too_big"] == trace["hit"] == 45 and (want[0] == INV).all() and not want[1].any()
    assert trace_alone["hit"] == 45 and (want_alone[0] == 3034).all() and (want_alone[1] == 2).all()
    assert len(case[0]) == 2 * len(alone[0]) and case[0].tobytes() != alone[0].tobytes()
    for c, w, tag in ((case, want, "too_big"), (alone, want_alone, "too_big_alone")):
        tsdf = _loaded(c[0], c[1])
        _equal(_render(tsdf, c), w, tag)
        tsdf.close()


def test_a_hit_that_is_too_far_is_invalid(viso):
    """!(v >= 1): a short focal length and baseline, the surface at 8.2 m."""
    case, want, trace = _want_traced("too_small")
    assert trace["hit_too_small"] == trace["hit"] == 45 and (want[0] == INV).all() and not want[1].any()
    tsdf = _loaded(case[0], case[1], log2=15)          # 12800 voxels
    _equal(_render(tsdf, case), want, "too_small")
    tsdf.close()


def test_a_hit_behind_the_camera_ends_the_march(viso):
    """!(zs > 0): the camera at the centre of a voxel of sum 0 inside a block; the rays that leave it into a negative voxel."""
    case, want, trace = _want_traced("behind")
    assert trace["hit_behind"] < trace["hit"] and trace["first_negative"] > 0
    _share(want[0], "behind")
    tsdf = _loaded(case[0], case[1])
    _equal(_render(tsdf, case), want, "behind")
    tsdf.close()


@pytest.mark.parametrize("name,value", [("gap_in", 7349), ("gap_out", 13973), ("gap_beside", None)])
def test_gaps(viso, name, value):
    """gap_in: gaps lead every ray, then the slab.  gap_out: the rays that pass the slab trail off in gaps.  gap_beside: nothing
    but empty voxels and gaps.  The casts of a sample's coordinates to int are defined only behind the range check."""
    case, want, trace = _want_traced(name)
    valid = want[0] != INV
    if value is None:
        assert trace["hit"] == 0 and not valid.any() and not want[1].any()
    else:
        assert trace["hit"] == valid.sum() > 0 and (want[0][valid] == value).all() and (want[1][valid] == 2).all()
        assert valid.all() == (name == "gap_in")
    tsdf = _loaded(case[0], case[1])
    _equal(_render(tsdf, case), want, name)
    tsdf.close()


def test_weights_and_means(viso):
    """The weight written is min(wa, wb) whichever is smaller, as uint32 up to 2^31; the means are quotients of doubles."""
    case, want, trace = _want_traced("weights_and_means")
    d, w = want
    valid = d != INV
    assert set(np.unique(w[valid]).tolist()) == {1, 2, 3, TT.BIG} and 0.5 < valid.mean() < 1.0
    assert len(np.unique(d[valid])) >= 5
    tsdf = _loaded(case[0], case[1])
    _equal(_render(tsdf, case), want, "weights_and_means")
    tsdf.close()


# ---- the crossings on the same kind of table -------------------------------------------------------------------------------------
def _crossings(tsdf, e, voxel, tag):
    n = []
    for mw in TT.BLOCK_MIN_WEIGHTS:
        want = R.crossings(e, mw)
        assert len(want) > 0, (tag, mw)
        got = tsdf.surface(mw)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (tag, mw, len(got), len(want))
        p, wp = tsdf.surface_points(mw), R.crossing_points(want, voxel)
        assert p.dtype == wp.dtype == np.float32 and p.shape == wp.shape and p.tobytes() == wp.tobytes(), (tag, mw)
        n.append(len(want))
    return n


@pytest.mark.parametrize("place", list(TT.CROSSING_PLACES))
def test_crossings_of_a_random_block(viso, place):
    """top: the voxels at 2^20 - 1 of an axis have no neighbour along it, and the kernel forms no key for one.  Neighbours that are
    absent or underweight at min_weight 2 and 3, sums of 0 (not negative) on either side."""
    e = TT.crossing_block(place)
    assert (e["sum"] == 0).any() and len({1, 2, 3} & set(e["weight"].tolist())) == 3
    last = (e["k"] == R.BIAS - 1)
    assert place != "top" or (last.any(axis=0).all() and last.all(axis=1).any())
    assert place != "bottom" or (e["k"] == -R.BIAS).any(axis=0).all()
    tsdf = _loaded(e, 0.2, log2=12)
    n = _crossings(tsdf, e, 0.2, place)
    print(f"{place}: {len(e)} voxels, {int(last.any(axis=1).sum())} with a last coordinate, {n} crossings at min_weight 1, 2, 3")
    assert n[0] > n[1] > n[2]
    tsdf.close()


@pytest.mark.parametrize("voxel", [0.05, 5.0])
def test_crossings_with_long_probe_chains(viso, voxel):
    """About 700 voxels in 2^10 slots: the three probes for the neighbours walk chains of tens of slots that wrap the table's end."""
    e = TT.chains_block()
    assert 680 <= len(e) <= 729 and (e["sum"] == 0).any()
    tsdf = _loaded(e, voxel, log2=10)
    n = _crossings(tsdf, e, voxel, ("chains", voxel))
    assert n[0] > n[1] > n[2]
    tsdf.close()
