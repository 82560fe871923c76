"""The TSDF map of include/viso_hip.h without a device: the two numpy restatements (tests/tsdf_ref.py) against each other, known
answers worked out by hand, a fronto-parallel wall, additivity, the struct layouts, the argument checks of the C ABI, the crossing
point, the PLY bytes, and the kernels' resource usage."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd import hostmath
from libviso_amd.abi import (TSDF_CROSSING_DTYPE, TSDF_DEFAULTS, TSDF_ENTRY_DTYPE, Param, TsdfCounters, TsdfParams)

import tsdf_ref as R
from estimator_util import kernel_resources
from test_speckle_cpu import random_map

INV = R.INVALID
POSE = np.linalg.inv(hostmath.tr2mat([0.013, -0.021, 0.007, 0.31, -0.12, 1.47]))


def _param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("seed", range(4))
def test_vectorised_equals_loop(seed):
    rng = np.random.default_rng(seed)
    rows, cols = int(rng.integers(1, 9)), int(rng.integers(1, 30))
    frames = [(random_map(rng, rows, cols, spread=2100, invalid=0.2), pose) for pose in (None, np.eye(4), POSE)]
    frames[0][0].flat[0] = 16 * 600          # a point 0.65 m ahead: samples with zj <= 0 at T = 8
    prm = _param()
    for voxel, trunc, md in ((0.05, 3, 16), (0.2, 1, 1), (0.2, 3, 16), (0.2, 8, 160), (1000.0, 2, 1)):
        a, sa = R.fuse(frames, prm, voxel, trunc, md)
        b, sb = R.fuse_loop(frames, prm, voxel, trunc, md)
        assert a.dtype == R.ENTRY and _same(a, b) and sa == sb and sa["n_out_of_range"] == 0 and sa["n_dropped"] == 0
        assert int(a["weight"].sum()) == sa["n_updates"] and (np.diff(R.keys_of(a["k"])) > 0).all()
        assert (np.abs(a["sum"]) <= trunc * 1024 * a["weight"].astype(np.int64)).all()
        assert _same(R.fuse(frames, prm, voxel, trunc, md, min_weight=2)[0], a[a["weight"] >= 2])
        ca = R.crossings(a)
        # the crossings of the vectorised form against a literal search
        table = {tuple(e["k"].tolist()): (int(e["weight"]), int(e["sum"])) for e in b}
        lit = []
        for k in sorted(table, key=lambda k: int(R.keys_of(np.array(k)))):
            for axis in range(3):
                n = tuple(k[i] + (i == axis) for i in range(3))
                if n in table and (table[k][1] < 0) != (table[n][1] < 0):
                    lit.append((k, axis, table[k][0], table[n][0], table[k][1], table[n][1]))
        assert _same(ca, np.array(lit, R.CROSSING) if lit else np.zeros(0, R.CROSSING)), (voxel, trunc)
    # an out-of-range sample is counted by both, and resets the duplicate rule in both
    far = np.eye(4); far[2, 3] = float(R.RANGE) * 0.2 / 1024 - 10.0
    a, sa = R.fuse([(frames[0][0], far)], prm, 0.2, 3, 16)
    b, sb = R.fuse_loop([(frames[0][0], far)], prm, 0.2, 3, 16)
    assert _same(a, b) and sa == sb and (sa["n_out_of_range"] > 0 or rows * cols < 20)


def _one_pixel(f, trunc, voxel=1.0):
    """One pixel on the optical axis at depth Z = f (base 1, d = 1 px, cu = cv = 0): X = Y = 0, so k = (0, 0, kz)."""
    prm = Param.default(base=1.0, f=f, cu=0.0, cv=0.0)
    m = np.full((3, 4), INV, np.int16)
    m[0, 0] = 16
    return [R.fuse([(m, None)], prm, voxel, trunc, 1), R.fuse_loop([(m, None)], prm, voxel, trunc, 1)]


def test_duplicate_rule_and_truncation_by_hand():
    """voxel 1 (s = 1 / 1024 and h = 0.5, both exact), T = 1: the samples are at zj = Z - 1, Z - 0.5, Z, Z + 0.5, Z + 1, the voxel of a
    sample is kz = floor(zj), its centre kz + 0.5, and q = floor((Z - kz - 0.5) 1024).
    Z = 2: kz = 1, 1, 2, 2, 3.  Voxel 1: q = 512; its second sample is a duplicate.  Voxel 2: q = -512; duplicate.  Voxel 3:
    q = -1536 < -1024: behind the surface by more than the truncation, no update.
    Z = 2.75: kz = 1, 2, 2, 3, 3.  Voxel 1: q = 1280, clamped to 1024.  Voxel 2: q = 256.  Voxel 3: q = -768."""
    for e, st in _one_pixel(2.0, 1):
        assert e["k"].tolist() == [[0, 0, 1], [0, 0, 2]] and e["weight"].tolist() == [1, 1] and e["sum"].tolist() == [512, -512]
        assert st == dict(n_points=1, n_updates=2, n_out_of_range=0, n_occupied=2, n_dropped=0)
        c = R.crossings(e)
        assert len(c) == 1 and c["k"][0].tolist() == [0, 0, 1] and c["axis"][0] == 2 and (c["wa"][0], c["wb"][0], c["sa"][0], c["sb"][0]) == (1, 1, 512, -512)
        # t = 512 / 1024: the crossing is half a voxel behind the centre of voxel 1, at the measured depth exactly
        assert R.crossing_points(c, 1.0).tolist() == [[0.5, 0.5, 2.0]]
    for e, st in _one_pixel(2.75, 1):
        assert e["k"].tolist() == [[0, 0, 1], [0, 0, 2], [0, 0, 3]] and e["sum"].tolist() == [1024, 256, -768] and st["n_updates"] == 3
        c = R.crossings(e)
        assert len(c) == 1 and c["k"][0].tolist() == [0, 0, 2] and R.crossing_points(c, 1.0).tolist() == [[0.5, 0.5, 2.75]]
    # a point nearer than the band: Z = 0.75, zj = -0.25, 0.25, 0.75, 1.25, 1.75: the first sample is not inserted;
    # kz = 0, 0, 1, 1: q = 256 (voxel 0), -768 (voxel 1)
    for e, st in _one_pixel(0.75, 1):
        assert e["k"].tolist() == [[0, 0, 0], [0, 0, 1]] and e["sum"].tolist() == [256, -768] and st["n_updates"] == 2 and st["n_out_of_range"] == 0
    # the invalid value, a disparity of 0 and one below min_disp16 contribute nothing
    m = np.array([[0, 15, INV, 16]], np.int16)
    e, st = R.fuse([(m, None)], Param.default(base=1.0, f=2.0, cu=0.0, cv=0.0), 1.0, 1, 16)
    assert st["n_points"] == 1 and st["n_updates"] == int(e["weight"].sum()) >= 2
    # more voxels than slots: the restatement reports drops
    wide = np.full((1, 1100), 16, np.int16)
    assert R.fuse([(wide, None)], Param.default(base=1.0, f=2.0, cu=0.0, cv=0.0), 0.5, 1, 1, capacity_log2=10)[1]["n_dropped"] > 0


@pytest.mark.parametrize("d16", [325, 115])
@pytest.mark.parametrize("voxel", [0.2, 0.05])
def test_fronto_parallel_wall(d16, voxel):
    """A constant map without a pose is a wall at Z0 = f base / d.  Every pixel that touches a voxel measures the same Z0 - zc, so
    the voxel's mean is the integer q = floor((Z0 - zc) / s), whatever its weight.  The centres of voxels adjacent along z differ
    by exactly 1024 s, so da - db is 1024 up to one unit of the floor: t 1024 = da 1024 / (da - db) is within one unit of da
    (|da| <= 1024), and da is within one unit of (Z0 - zc_a) / s.  Hence |p_z - Z0| <= 2 s, plus the one rounding of p_z to float32
    (half an ulp: |p_z| 2^-24).  Voxels adjacent along x or y have the same zc, hence the same sign: every crossing has axis 2."""
    prm = _param()
    m = np.full((37, 333), d16, np.int16)
    e, st = R.fuse([(m, None)], prm, voxel, 3, 16)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0 and st["n_points"] == m.size
    c = R.crossings(e)
    Z0 = prm.f * prm.base / (d16 / 16.0)
    p = R.crossing_points(c, voxel).astype(np.float64)
    s = voxel / 1024.0
    err = np.abs(p[:, 2] - Z0)
    print(f"disp16 {d16}, voxel {voxel}: {len(e)} voxels, {len(c)} crossings, worst |p_z - Z0| = {err.max() / s:.3f} s")
    assert len(c) > 0 and (c["axis"] == 2).all()
    assert (e["sum"] % e["weight"].astype(np.int64) == 0).all()
    assert (err <= 2.0 * s + np.abs(p[:, 2]) * 2.0 ** -24).all()


def test_additivity_of_the_restatement():
    rng = np.random.default_rng(5)
    prm = _param()
    poses = [None, np.eye(4), POSE, POSE @ POSE, np.linalg.inv(POSE)]
    frames = [(random_map(rng, 9, 31, spread=1500, invalid=0.3), p) for p in poses]
    whole, st = R.fuse(frames, prm, 0.2, 3, 16)
    assert st["n_out_of_range"] == 0 and len(R.crossings(whole)) > 0
    assert _same(R.fuse(frames[::-1], prm, 0.2, 3, 16)[0], whole)
    for cut in (1, 2, 4):
        a, b = R.fuse(frames[:cut], prm, 0.2, 3, 16)[0], R.fuse(frames[cut:], prm, 0.2, 3, 16)[0]
        assert _same(R.merge(a, b), whole) and _same(R.merge(b, a), whole)
    parts = [R.fuse([fr], prm, 0.2, 3, 16)[0] for fr in frames]
    assert _same(R.merge(*parts), whole) and _same(R.merge(*parts[::-1]), whole) and _same(R.merge(whole), whole)
    assert _same(R.crossings(R.merge(*parts), 2), R.crossings(whole, 2))


def test_struct_layouts_and_defaults():
    assert R.ENTRY == TSDF_ENTRY_DTYPE and TSDF_ENTRY_DTYPE.itemsize == 24
    assert [TSDF_ENTRY_DTYPE.fields[n][1] for n in ("k", "weight", "sum")] == [0, 12, 16]
    assert R.CROSSING == TSDF_CROSSING_DTYPE and TSDF_CROSSING_DTYPE.itemsize == 40
    assert [TSDF_CROSSING_DTYPE.fields[n][1] for n in ("k", "axis", "wa", "wb", "sa", "sb")] == [0, 12, 16, 20, 24, 32]
    assert [(f[0], getattr(TsdfParams, f[0]).offset) for f in TsdfParams._fields_] == [("voxel", 0), ("trunc_voxels", 8), ("min_disp16", 12),
                                                                                      ("capacity_log2", 16)]
    assert C.sizeof(TsdfParams) == 24 and C.sizeof(TsdfCounters) == 40
    assert [f[0] for f in TsdfCounters._fields_] == ["n_points", "n_updates", "n_out_of_range", "n_dropped", "n_occupied"]
    L = libviso_amd.load()
    p = TsdfParams(-1.0, -1, -1, -1)
    L.viso_tsdf_params_default(C.byref(p))
    assert (p.voxel, p.trunc_voxels, p.min_disp16, p.capacity_log2) == (0.2, 3, 16, 26)
    assert TSDF_DEFAULTS == dict(voxel=0.2, trunc_voxels=3, min_disp16=16, capacity_log2=26)
    L.viso_tsdf_params_default(None)
    q = libviso_amd.tsdf_params(voxel=0.05, trunc_voxels=8)
    assert (q.voxel, q.trunc_voxels, q.min_disp16, q.capacity_log2) == (0.05, 8, 16, 26) and q.ok()
    with pytest.raises(TypeError):
        libviso_amd.tsdf_params(foo=1)


def test_argument_errors_without_a_device():
    L = libviso_amd.load()
    h = C.c_void_p()
    ok = libviso_amd.tsdf_params()
    assert L.viso_tsdf_create(None, None, C.byref(h)) == -1 and L.viso_tsdf_create(None, C.byref(ok), None) == -1
    for bad in (dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(trunc_voxels=0),
                dict(trunc_voxels=9), dict(min_disp16=0), dict(capacity_log2=9), dict(capacity_log2=29)):
        p = libviso_amd.tsdf_params(**bad)
        assert not p.ok() and L.viso_tsdf_create(None, C.byref(p), C.byref(h)) == -1 and h.value is None, bad
        assert b"viso_tsdf_create" in L.viso_last_error()
    assert L.viso_tsdf_create(C.c_void_p(12345), C.byref(ok), C.byref(h)) == -1     # not a context
    # a handle that is not a TSDF map: every call answers, none follows the pointer
    fake = C.c_void_p(4096)
    m = np.zeros((4, 5), np.int16)
    mp = m.ctypes.data_as(C.POINTER(C.c_int16))
    prm = _param()
    n = C.c_size_t()
    e = np.zeros(1, TSDF_ENTRY_DTYPE); e["weight"] = 1
    cr = np.zeros(1, TSDF_CROSSING_DTYPE)
    st = TsdfCounters()
    T = np.eye(4)
    Tp = T.ctypes.data_as(C.POINTER(C.c_double))
    for handle in (None, fake):
        assert L.viso_tsdf_clear(handle) == -1
        assert L.viso_tsdf_fuse(handle, mp, 4, 5, C.byref(prm), None) == -1
        assert L.viso_tsdf_add_entries(handle, e.ctypes.data, 1) == -1
        assert L.viso_tsdf_count(handle, 1, C.byref(n)) == -1
        assert L.viso_tsdf_get(handle, 1, e.ctypes.data, 1, C.byref(n)) == -1
        assert L.viso_tsdf_surface_count(handle, 1, C.byref(n)) == -1
        assert L.viso_tsdf_surface(handle, 1, cr.ctypes.data, 1, C.byref(n)) == -1
        assert L.viso_tsdf_stats(handle, C.byref(st)) == -1
        assert L.viso_batch_fuse_tsdf(None, handle, 0, 1, Tp) == -1
    assert b"viso_batch_fuse_tsdf" in L.viso_last_error()
    assert L.viso_tsdf_destroy(None) == 1 and L.viso_tsdf_destroy(fake) == -1
    assert b"viso_tsdf_destroy" in L.viso_last_error()
    # the crossing point's own checks
    out = np.zeros(3, np.float32)
    op = out.ctypes.data_as(C.POINTER(C.c_float))
    good = np.zeros(1, TSDF_CROSSING_DTYPE)
    good["wa"], good["wb"], good["sa"], good["sb"] = 1, 1, 5, -5
    assert L.viso_tsdf_crossing_point(good.ctypes.data, 0.2, op) == 1
    assert L.viso_tsdf_crossing_point(None, 0.2, op) == -1 and L.viso_tsdf_crossing_point(good.ctypes.data, 0.2, None) == -1
    assert L.viso_tsdf_crossing_point(good.ctypes.data, 0.0, op) == -1 and L.viso_tsdf_crossing_point(good.ctypes.data, float("nan"), op) == -1
    for field, value in (("axis", 3), ("axis", -1), ("wa", 0), ("wb", 0), ("sb", 5), ("sb", 0), ("sa", -5)):
        bad = good.copy()
        bad[field] = value
        assert L.viso_tsdf_crossing_point(bad.ctypes.data, 0.2, op) == -1, (field, value)
    assert b"viso_tsdf_crossing_point" in L.viso_last_error()
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        libviso_amd.TsdfMap(voxel=-1.0)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        libviso_amd.TsdfMap(trunc_voxels=9)
    with pytest.raises(TypeError):
        libviso_amd.TsdfMap(params=libviso_amd.tsdf_params(), voxel=0.1)


def _random_crossings(rng, n):
    c = np.zeros(n, TSDF_CROSSING_DTYPE)
    c["k"] = rng.integers(-R.BIAS, R.BIAS - 1, (n, 3))
    c["k"][:4] = [[-R.BIAS] * 3, [R.BIAS - 2] * 3, [0, 0, 0], [-1, -1, -1]]
    c["axis"] = rng.integers(0, 3, n)
    c["wa"] = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    c["wb"] = rng.integers(1, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    c["wa"][:6] = [1, 1, 3, 7, 2 ** 32 - 1, 2]
    sign = np.where(rng.random(n) < 0.5, 1, -1)
    fa, fb = rng.random(n), rng.random(n)
    c["sa"] = np.floor(fa * 8 * 1024 * c["wa"]).astype(np.int64)
    c["sb"] = -np.floor(fb * 8 * 1024 * c["wb"]).astype(np.int64) - 1
    swap = sign < 0                      # a negative, b not
    c["sa"][swap], c["sb"][swap] = -c["sa"][swap] - 1, -c["sb"][swap] - 1
    c["sa"][0], c["sb"][0] = 0, -1       # a sum of zero counts as not negative
    return c


def test_crossing_point_equals_restatement_bit_for_bit():
    c = _random_crossings(np.random.default_rng(11), 3000)
    assert ((c["sa"] < 0) != (c["sb"] < 0)).all()
    for voxel in (0.05, 0.2, 1.0, 1000.0, 1e-3):
        got = libviso_amd.tsdf_crossing_points(c, voxel)
        want = R.crossing_points(c, voxel)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), voxel
    # the crossing lies between the two centres (up to the one rounding to float32)
    p = R.crossing_points(c, 0.2).astype(np.float64)
    i = np.arange(len(c))
    lo = (c["k"][i, c["axis"]] + 0.5) * 0.2
    assert (p[i, c["axis"]] >= lo - 1e-2).all() and (p[i, c["axis"]] <= lo + 0.2 + 1e-2).all()


def test_ply_header_and_bytes(tmp_path):
    rng = np.random.default_rng(2)
    e, _ = R.fuse([(random_map(rng, 12, 40, spread=1500, invalid=0.2), POSE)], _param(), 0.2, 3, 16)
    c = R.crossings(e)
    assert len(c) > 10
    data = R.ply_bytes(c, 0.2)
    head, _, body = data.partition(b"end_header\n")
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0" and f"element vertex {len(c)}" in lines
    assert [ln for ln in lines if ln.startswith("property")] == ["property float x", "property float y", "property float z", "property uint weight"]
    assert len(body) == 16 * len(c)
    v = np.frombuffer(body, np.dtype([("xyz", "<f4", (3,)), ("weight", "<u4")]))
    assert np.array_equal(v["xyz"], R.crossing_points(c, 0.2)) and np.array_equal(v["weight"], np.minimum(c["wa"], c["wb"]))
    assert libviso_amd.surface_ply_bytes(c, 0.2) == data
    f = tmp_path / "s.ply"
    libviso_amd.write_surface_ply(str(f), c, 0.2)
    assert f.read_bytes() == data
    assert R.ply_bytes(c[:0], 0.2).endswith(b"element vertex 0\nproperty float x\nproperty float y\nproperty float z\nproperty uint weight\nend_header\n")


def test_kernels_have_no_scratch():
    shared = ("add_entries", "compact", "clear", "evict_mark", "evict_rebuild", "evict_sweep")   # voxel_hash.h's templates, by mangled name
    names = ("tsdf_fuse_kernel", "tsdf_crossings_kernel") + tuple(f"voxel_{k}_kernelI11TsdfPayloadILb0EE" for k in shared)
    res = kernel_resources("tsdf.hip", names)
    for name, (occ, scratch) in res.items():
        print(f"{name}: occupancy {occ}, scratch {scratch}")
        assert scratch == 0 and occ >= 1


def test_device_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(libviso_amd.VisoError, match="-2"):
        libviso_amd.TsdfMap(voxel=0.2, capacity_log2=10)
