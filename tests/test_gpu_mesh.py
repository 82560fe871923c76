"""The triangle mesh of the TSDF map on the device (include/viso_hip.h, viso_tsdf_mesh / viso_tsdf_mesh_count; tsdf_mesh_kernel in
libviso_amd/csrc/tsdf.hip) against its numpy restatement (tests/mesh_ref.py), bit for bit on the sorted vertex array and the
triangle array.  The restatement derives every tetrahedron's triangles from the geometric rule and holds no table of cases; the
kernel holds the table: their agreement is the test of the table.

The restatement is fed the entries of tests/tsdf_ref.py (or the hand-made ones), not what the device read back; that the device's
entries equal them is asserted beside it."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import TSDF_ENTRY_DTYPE, TSDF_MESH_VERTEX_DTYPE, Param

import disparity_ref as DR
import mesh_ref as MR
import tsdf_ref as R
from test_gpu_tsdf import POSE, _mixed_map
from tsdf_tables import random_block as _random_block

pytestmark = pytest.mark.gpu

LOG2 = 21


def _param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _counts(tsdf, min_weight=1):
    nv, nt = C.c_size_t(), C.c_size_t()
    assert tsdf.L.viso_tsdf_mesh_count(tsdf.h, min_weight, C.byref(nv), C.byref(nt)) == 1
    return nv.value, nt.value


def _check(tsdf, entries, tag, min_weights=(1,)):
    """The device mesh of the map equals the restatement over `entries`; returns the number of triangles seen."""
    assert _same(tsdf.entries(), entries), tag
    n = 0
    for mw in min_weights:
        v, t = tsdf.mesh(mw)
        wv, wt = MR.mesh(entries, tsdf.voxel, mw)
        assert v.dtype == TSDF_MESH_VERTEX_DTYPE == MR.VERTEX and t.dtype == np.uint32 and t.shape == (len(t), 3)
        assert (len(v), len(t)) == (len(wv), len(wt)) == _counts(tsdf, mw), (tag, mw, len(v), len(t), len(wv), len(wt))
        assert _same(t, wt), (tag, mw)
        assert np.array_equal(v["k"], wv["k"]) and np.array_equal(v["dir"], wv["dir"]) and np.array_equal(v["weight"], wv["weight"]), (tag, mw)
        assert np.array_equal(v["p"].view(np.uint32), wv["p"].view(np.uint32)), (tag, mw)
        assert _same(v, wv), (tag, mw)
        n += len(t)
    return n


def test_sphere_through_add_entries(viso):
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=13)
    assert tsdf.mesh()[0].shape == (0,) and tsdf.mesh()[1].shape == (0, 3) and _counts(tsdf) == (0, 0)      # the empty map
    e = MR.sphere_entries(weight=2)
    tsdf.add_entries(e)
    before = (tsdf.entries().tobytes(), tsdf.surface().tobytes(), tsdf.stats())
    assert _check(tsdf, e, "sphere", (1, 2)) == 2 * 1512
    assert tsdf.mesh(3)[1].shape == (0, 3) and _counts(tsdf, 3) == (0, 0)
    v, t = tsdf.mesh()
    ok, n_edges = MR.closed_and_oriented(t)
    assert ok and len(v) - n_edges + len(t) == 2 and (len(v), len(t)) == (758, 1512)
    # nothing of the map changes by meshing it
    assert before == (tsdf.entries().tobytes(), tsdf.surface().tobytes(), tsdf.stats())
    # the checks behind a live handle, before any launch
    L = tsdf.L
    nv, nt = C.c_size_t(5), C.c_size_t(5)
    vb, tb = np.zeros(len(v), TSDF_MESH_VERTEX_DTYPE), np.zeros((len(t), 3), np.uint32)
    assert L.viso_tsdf_mesh_count(tsdf.h, 0, C.byref(nv), C.byref(nt)) == -1
    assert L.viso_tsdf_mesh_count(tsdf.h, 1, None, C.byref(nt)) == -1 and L.viso_tsdf_mesh_count(tsdf.h, 1, C.byref(nv), None) == -1
    assert L.viso_tsdf_mesh(tsdf.h, 0, vb.ctypes.data, len(vb), tb.ctypes.data, len(tb), C.byref(nv), C.byref(nt)) == -1
    assert L.viso_tsdf_mesh(tsdf.h, 1, None, len(vb), tb.ctypes.data, len(tb), C.byref(nv), C.byref(nt)) == -1
    assert L.viso_tsdf_mesh(tsdf.h, 1, vb.ctypes.data, len(vb), None, len(tb), C.byref(nv), C.byref(nt)) == -1
    assert L.viso_tsdf_mesh(tsdf.h, 1, vb.ctypes.data, len(vb), tb.ctypes.data, len(tb), None, C.byref(nt)) == -1
    assert (nv.value, nt.value) == (5, 5) and b"viso_tsdf_mesh" in L.viso_last_error()
    # a capacity that is too small: the code, both numbers, nothing written
    for cv, ct in ((len(v) - 1, len(t)), (len(v), len(t) - 1), (0, 0)):
        nv, nt = C.c_size_t(), C.c_size_t()
        assert L.viso_tsdf_mesh(tsdf.h, 1, vb.ctypes.data, cv, tb.ctypes.data, ct, C.byref(nv), C.byref(nt)) == -1
        assert (nv.value, nt.value) == (len(v), len(t)) and not vb["weight"].any() and not tb.any()
    assert L.viso_tsdf_mesh(tsdf.h, 1, vb.ctypes.data, len(vb), tb.ctypes.data, len(tb), C.byref(nv), C.byref(nt)) == 1
    assert _same(vb, v) and _same(tb, t)
    tsdf.close()


@pytest.mark.parametrize("place", ["origin", "top", "bottom"])
def test_random_block(viso, place):
    """9^3 voxels at 70 % occupancy, so that most cells are incomplete and edges belong to complete cells other than their owner's;
    weights 1..3 against min_weight 1..3; sums of 0 and at both ends of the band.  top: the block's last voxels are the last of
    every axis (2^20 - 1), where no cell exists and no neighbour key is formed; bottom: its first are the first (-2^20)."""
    rng = np.random.default_rng(9)
    origin = {"origin": -4, "top": R.BIAS - 9, "bottom": -R.BIAS}[place]
    e = _random_block(rng, origin=origin)
    assert (e["sum"] == 0).any() and (np.abs(e["sum"]) == 3 * 1024 * e["weight"].astype(np.int64)).any()
    assert place != "top" or (e["k"] == R.BIAS - 1).any()
    tsdf = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=12)
    tsdf.add_entries(e)
    n = _check(tsdf, e, place, (1, 2, 3))
    print(f"{place}: {len(e)} voxels, {n} triangles over min_weight 1, 2, 3")
    assert n > 100
    tsdf.close()


def test_long_probe_chains(viso):
    """About 700 voxels in the smallest table (2^10 slots): chains of tens of slots that wrap the table's end."""
    rng = np.random.default_rng(10)
    e = _random_block(rng, occupancy=0.96)
    assert 680 <= len(e) <= 729
    for voxel in (0.05, 5.0):
        tsdf = libviso_amd.TsdfMap(None, voxel=voxel, capacity_log2=10)
        tsdf.add_entries(e)
        assert _check(tsdf, e, "chains", (1, 2)) > 500
        tsdf.close()


@pytest.mark.parametrize("shape", [(37, 333), (3, 130)])
@pytest.mark.parametrize("trunc", [1, 3, 8])
def test_fused_maps(viso, shape, trunc):
    rng = np.random.default_rng(shape[0] * 3 + shape[1] + trunc)
    m = _mixed_map(rng, *shape)
    prm = _param()
    n = 0
    for voxel in (0.05, 0.2, 5.0):
        tsdf = libviso_amd.TsdfMap(None, voxel=voxel, trunc_voxels=trunc, capacity_log2=LOG2)
        for name, pose in (("none", None), ("rigid", POSE)):
            want, st = R.fuse([(m, pose)], prm, voxel, trunc, 16, LOG2)
            assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0
            tsdf.clear()
            tsdf.fuse(m, prm, pose=pose)
            surface = tsdf.surface().tobytes()
            n += _check(tsdf, want, (shape, trunc, voxel, name), (1, 2))
            assert tsdf.surface().tobytes() == surface == R.crossings(want).tobytes()
        tsdf.close()
    print(f"{shape}, T {trunc}: {n} triangles")
    assert n > 1000 or shape[0] == 3          # three rows are too thin for complete cells: every vertex record is dropped


@pytest.mark.parametrize("method", ["bm", "sgm"])
def test_maps_of_both_methods(viso, method):
    L, Rimg, _ = DR.slanted_pair()
    raw = libviso_amd.stereo_disparity(L, Rimg) if method == "bm" else libviso_amd.stereo_sgm(L, Rimg)
    prm = _param()
    tsdf = libviso_amd.TsdfMap(None, capacity_log2=LOG2)
    for pose in (None, POSE):
        want, st = R.fuse([(raw, pose)], prm, capacity_log2=LOG2)
        assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0
        tsdf.clear()
        tsdf.fuse(raw, prm, pose=pose)
        n = _check(tsdf, want, method, (1, 2))
        v, t = tsdf.mesh()
        print(f"{method}: {len(want)} voxels, {len(v)} vertices, {len(t)} triangles")
        assert n > 1000
    tsdf.close()


def test_partitions_joined_by_add_entries(viso):
    whole = MR.sphere_entries(weight=3)
    a, b = libviso_amd.TsdfMap(None, capacity_log2=13), libviso_amd.TsdfMap(None, capacity_log2=13)
    # the same voxels in both parts: weights and sums add
    a.add_entries(MR.sphere_entries(weight=1))
    b.add_entries(MR.sphere_entries(weight=2))
    a.add_entries(b.entries())
    assert _check(a, whole, "summed", (1, 3)) == 2 * 1512
    # disjoint parts, each with holes where the other one's voxels are
    a.clear(); b.clear()
    pick = np.random.default_rng(4).random(len(whole)) < 0.5
    a.add_entries(whole[pick]); b.add_entries(whole[~pick])
    assert len(a.mesh()[1]) < 1512
    b.add_entries(a.entries())
    assert _check(b, whole, "joined") == 1512
    one = libviso_amd.TsdfMap(None, capacity_log2=13)
    one.add_entries(whole)
    assert all(_same(x, y) for x, y in zip(one.mesh(), b.mesh()))
    for m in (a, b, one):
        m.close()


def test_overflow_refuses_and_clear_recovers(viso):
    tsdf = libviso_amd.TsdfMap(None, capacity_log2=10)
    many = np.zeros(1500, TSDF_ENTRY_DTYPE)
    many["k"][:, 0] = np.arange(1500) + 500
    many["weight"], many["sum"] = 1, -7
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.add_entries(many)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        tsdf.mesh()
    nv, nt = C.c_size_t(), C.c_size_t()
    assert tsdf.L.viso_tsdf_mesh_count(tsdf.h, 1, C.byref(nv), C.byref(nt)) == -4
    tsdf.clear()
    assert _counts(tsdf) == (0, 0)
    e = _random_block(np.random.default_rng(12))
    tsdf.add_entries(e)
    assert _check(tsdf, e, "after clear") > 100
    tsdf.close()


def test_map_that_outlives_its_context(viso):
    ctx = libviso_amd.Context(0)
    tsdf = libviso_amd.TsdfMap(ctx, capacity_log2=13)
    e = MR.sphere_entries()
    tsdf.add_entries(e)
    assert _check(tsdf, e, "own context") == 1512
    ctx.close()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        tsdf.mesh()
    nv, nt = C.c_size_t(), C.c_size_t()
    assert tsdf.L.viso_tsdf_mesh_count(tsdf.h, 1, C.byref(nv), C.byref(nt)) == -1
    tsdf.close()
    assert tsdf.h is None
