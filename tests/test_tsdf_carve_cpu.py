"""The TSDF fuse options of include/viso_hip.h ("TSDF fuse options": free-space carving, disparity-based weights) without a device:
the two numpy restatements (tests/carve_ref.py) against each other and, at the defaults, against tests/tsdf_ref.py and
tests/gray_ref.py; the weight formula and one pixel worked out by hand; the ghost that carving removes and the wall that weights
move; additivity; the options' prototypes and defaults, the argument checks of the two calls, and the extended kernels' resource usage."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd import hostmath
from libviso_amd.abi import PROTOTYPES, TSDF_FUSE_DEFAULTS, Param

import carve_ref as CR
import gray_ref as G
import tsdf_ref as R
from estimator_util import kernel_resources
from test_speckle_cpu import random_map

INV = R.INVALID
POSE = np.linalg.inv(hostmath.tr2mat([0.013, -0.021, 0.007, 0.31, -0.12, 1.47]))
BOTH = dict(carve_voxels=6, weight_shift=12, weight_max=255)
OPTIONS = (dict(carve_voxels=6), dict(weight_shift=12, weight_max=255), BOTH, dict(carve_voxels=9, carve_near=1.3, weight_shift=8, weight_max=77))


def _param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _clean(st):
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0, st
    return st


@pytest.mark.parametrize("seed", range(3))
def test_vectorised_equals_loop(seed):
    rng = np.random.default_rng(seed)
    rows, cols = int(rng.integers(1, 7)), int(rng.integers(1, 24))
    frames = [(random_map(rng, rows, cols, spread=2100, invalid=0.2), pose) for pose in (None, POSE)]
    frames[0][0].flat[0] = 16 * 600          # a point 0.65 m ahead: nearer than the carved length
    images = [rng.integers(0, 256, (rows, cols)).astype(np.uint8) for _ in frames]
    gframes = [(m, im, pose) for (m, pose), im in zip(frames, images)]
    prm = _param()
    for voxel, trunc, md in ((0.05, 3, 16), (0.2, 1, 1), (0.2, 8, 160)):
        for o in OPTIONS:
            a, sa = CR.fuse(frames, prm, voxel, trunc, md, **o)
            b, sb = CR.fuse_loop(frames, prm, voxel, trunc, md, **o)
            _clean(sa)
            assert a.dtype == R.ENTRY and _same(a, b) and sa == sb, (voxel, trunc, o)
            assert (np.diff(R.keys_of(a["k"])) > 0).all() and int(a["weight"].sum()) >= sa["n_updates"]
            if o.get("weight_shift") is None:
                assert int(a["weight"].sum()) == sa["n_updates"]
            # what viso_tsdf_add_entries checks holds by construction
            assert (np.abs(a["sum"]) <= trunc * 1024 * a["weight"].astype(np.int64)).all()
            ga, gsa = CR.fuse(gframes, prm, voxel, trunc, md, gray=True, **o)
            gb, gsb = CR.fuse_loop(gframes, prm, voxel, trunc, md, gray=True, **o)
            assert ga.dtype == G.ENTRY and _same(ga, gb) and gsa == gsb == sa and _same(G.plain(ga), a)
            assert G.entry_ok(ga, trunc).all()


def test_default_options_are_the_plain_restatements():
    rng = np.random.default_rng(130)
    m = random_map(rng, 5, 130, spread=2100, invalid=0.2)
    image = rng.integers(0, 256, m.shape).astype(np.uint8)
    prm = _param()
    for pose in (None, POSE):
        for voxel, trunc in ((0.2, 3), (0.05, 8), (5.0, 1)):
            want, st = R.fuse([(m, pose)], prm, voxel, trunc, 16)
            for got, gst in (CR.fuse([(m, pose)], prm, voxel, trunc, 16), CR.fuse_loop([(m, pose)], prm, voxel, trunc, 16),
                             CR.fuse([(m, pose)], prm, voxel, trunc, 16, **CR.DEFAULTS)):
                assert _same(got, want) and gst == st
            gwant, gst = G.fuse([(m, image, pose)], prm, voxel, trunc, 16)
            got, st2 = CR.fuse([(m, image, pose)], prm, voxel, trunc, 16, gray=True)
            assert _same(got, gwant) and st2 == gst
    # carve_near alone changes nothing: without carving there is no free-space sample
    assert _same(CR.fuse([(m, POSE)], prm, carve_near=30.0)[0], R.fuse([(m, POSE)], prm)[0])


def test_weight_formula_by_hand():
    """w = min(max(d16^2 >> shift, 1), weight_max).  16^2 = 2^8, 63^2 = 3969, 64^2 = 2^12, 65^2 = 4225, 1023^2 = 1046529 = 255.5 x 2^12,
    1024^2 = 2^20, 32767^2 = 1073676289 = 2^30 - 65535."""
    d16 = [16, 63, 64, 65, 1023, 1024, 32767]
    table = {
        (0, 255): [255, 255, 255, 255, 255, 255, 255],             # the upper clamp everywhere: 16^2 = 256 already
        (0, 1): [1, 1, 1, 1, 1, 1, 1],
        (12, 255): [1, 1, 1, 1, 255, 255, 255],                    # 0 -> 1 (the lower clamp), 0 -> 1, 1, 1, 255, 256 -> 255, 262127 -> 255
        (12, 7): [1, 1, 1, 1, 7, 7, 7],
        (8, 255): [1, 15, 16, 16, 255, 255, 255],
        (30, 255): [1, 1, 1, 1, 1, 1, 1],                          # 32767^2 < 2^30: the lower clamp everywhere
    }
    for (shift, wmax), want in table.items():
        assert [CR.weight_of(d, shift, wmax) for d in d16] == want, (shift, wmax)
        assert CR.weights_of(np.array(d16, np.int16), shift, wmax).tolist() == want, (shift, wmax)
    assert [CR.weight_of(d) for d in d16] == [1] * 7 and CR.weights_of(np.array(d16, np.int16)).tolist() == [1] * 7
    # the unclamped middle: proportional to 1 / Z^2
    assert CR.weight_of(400, 12) == 39 and CR.weight_of(800, 12) == 156


def _one_pixel(f, trunc, voxel=1.0, **o):
    """One pixel on the optical axis at depth Z = f (base 1, d = 1 px, cu = cv = 0): X = Y = 0, so k = (0, 0, kz)."""
    prm = Param.default(base=1.0, f=f, cu=0.0, cv=0.0)
    m = np.full((3, 4), INV, np.int16)
    m[0, 0] = 16
    return prm, [CR.fuse([(m, None)], prm, voxel, trunc, 1, **o), CR.fuse_loop([(m, None)], prm, voxel, trunc, 1, **o)]


def test_one_pixel_by_hand():
    """voxel 1 (s = 1 / 1024, h = 0.5), T = 1, C = 2: j = -6 .. 2, zj = Z + j / 2, kz = floor(zj), q = floor((Z - kz - 0.5) 1024).
    Z = 4.25: zj = 1.25, 1.75 | 2.25, 2.75 | 3.25, 3.75 | 4.25, 4.75 | 5.25; the first four are free-space samples.
    Voxel 1: q = 2816 -> 1024; voxel 2: 1792 -> 1024; voxel 3: 768; voxel 4: -256; voxel 5: -1280 < -1024, no update."""
    prm, both = _one_pixel(4.25, 1, carve_voxels=2)
    for e, st in both:
        assert e["k"].tolist() == [[0, 0, 1], [0, 0, 2], [0, 0, 3], [0, 0, 4]] and e["weight"].tolist() == [1, 1, 1, 1]
        assert e["sum"].tolist() == [1024, 1024, 768, -256]
        assert st == dict(n_points=1, n_updates=4, n_out_of_range=0, n_occupied=4, n_dropped=0)
    assert CR.samples(16, 0, 0, prm, None, 1.0, 1, carve_voxels=2) == [
        (-6, (0, 0, 1), 1024, 1), (-4, (0, 0, 2), 1024, 1), (-2, (0, 0, 3), 768, 1), (0, (0, 0, 4), -256, 1), (2, (0, 0, 5), None, 1)]
    # without carving: the band alone
    assert _one_pixel(4.25, 1)[1][0][0]["k"].tolist() == [[0, 0, 3], [0, 0, 4]]
    # with a weight: 16^2 >> 4 = 16 on every sample, the free-space ones included; the counters count updates
    for e, st in _one_pixel(4.25, 1, carve_voxels=2, weight_shift=4)[1]:
        assert e["weight"].tolist() == [16] * 4 and e["sum"].tolist() == [16384, 16384, 12288, -4096] and st["n_updates"] == 4
    # carve_near = 1.5 cuts exactly the sample at zj = 1.25: voxel 1 is then entered by its second sample, the map is the same
    s = CR.samples(16, 0, 0, prm, None, 1.0, 1, carve_voxels=2, carve_near=1.5)
    assert s[:2] == [(-6, None, None, 1), (-5, (0, 0, 1), 1024, 1)] and s[2:] == CR.samples(16, 0, 0, prm, None, 1.0, 1, carve_voxels=2)[1:]
    assert _same(_one_pixel(4.25, 1, carve_voxels=2, carve_near=1.5)[1][0][0], both[0][0])
    # zj = 1.75 is not nearer than carve_near = 1.75: still inserted; 1.76 cuts both samples of voxel 1; 2.75 leaves only the band,
    # since the test is on free-space samples alone and the band's first sample lies at 3.25
    assert _one_pixel(4.25, 1, carve_voxels=2, carve_near=1.75)[1][1][0]["k"][:, 2].tolist() == [1, 2, 3, 4]
    assert _one_pixel(4.25, 1, carve_voxels=2, carve_near=1.76)[1][1][0]["k"][:, 2].tolist() == [2, 3, 4]
    for e, st in _one_pixel(4.25, 1, carve_voxels=2, carve_near=2.76)[1] + _one_pixel(4.25, 1, carve_voxels=2, carve_near=100.0)[1]:
        assert e["k"][:, 2].tolist() == [3, 4] and e["sum"].tolist() == [768, -256]
    # a pixel nearer than the carved length: Z = 0.75, zj = -2.25 .. -0.25 (j = -6 .. -2) are not inserted, then 0.25, 0.75 | 1.25,
    # 1.75: voxel 0: q = 256, voxel 1: q = -768, the map without carving
    for e, st in _one_pixel(0.75, 1, carve_voxels=2)[1]:
        assert e["k"].tolist() == [[0, 0, 0], [0, 0, 1]] and e["sum"].tolist() == [256, -768] and st["n_updates"] == 2 and st["n_out_of_range"] == 0
    assert [s[1] for s in CR.samples(16, 0, 0, Param.default(base=1.0, f=0.75, cu=0.0, cv=0.0), None, 1.0, 1, carve_voxels=2)[:5]] == [None] * 5


# ---- the ghost scene: a patch at 5 m in one frame, then three frames of a wall at 10 m seen through it --------------------------------
GHOST_VOXEL, GHOST_TRUNC = 0.2, 3


def ghost_frames():
    prm = _param()

    def d16_of(Z):
        return int(round(prm.f * prm.base / Z * 16.0))
    patch = np.full((24, 192), INV, np.int16)
    patch[8:16, 64:128] = d16_of(5.0)
    wall = np.full((24, 192), d16_of(10.0), np.int16)
    return prm, [(patch, None)] + [(wall.copy(), None) for _ in range(3)], d16_of(5.0), d16_of(10.0)


def ghost_counts(entries, min_weight):
    """(crossings, their points' z) of a ghost scene's entries."""
    c = R.crossings(entries, min_weight)
    return c, R.crossing_points(c, GHOST_VOXEL)[:, 2].astype(np.float64)


def check_ghost(plain_entries, carved_entries):
    """The assertions of the ghost scene on the entries fused with C = 0 and with a C that reaches the patch."""
    for mw in (1, 2):
        c0, z0 = ghost_counts(plain_entries, mw)
        c1, z1 = ghost_counts(carved_entries, mw)
        print(f"min_weight {mw}: C = 0: {int(((z0 > 4) & (z0 < 6)).sum())} crossings at 5 m, {int(((z0 > 9) & (z0 < 11)).sum())} at 10 m; "
              f"carved: {int((z1 < 9).sum())} nearer than 9 m, {int(((z1 > 9) & (z1 < 11)).sum())} at 10 m")
        assert ((z0 > 4) & (z0 < 6)).sum() > 0 and ((z0 > 9) & (z0 < 11)).sum() > 0
        assert (z1 < 9).sum() == 0
        far0, far1 = c0[(z0 > 9) & (z0 < 11)], c1[(z1 > 9) & (z1 < 11)]
        assert _same(far0["k"], far1["k"]) and _same(far0["axis"], far1["axis"])
        assert np.array_equal(R.crossing_points(far0, GHOST_VOXEL).view(np.uint32), R.crossing_points(far1, GHOST_VOXEL).view(np.uint32))


@pytest.mark.parametrize("carve", [28, 40])
def test_ghost_scene(carve):
    prm, frames, _, _ = ghost_frames()
    e0, st0 = CR.fuse(frames, prm, GHOST_VOXEL, GHOST_TRUNC, 16)
    e1, st1 = CR.fuse(frames, prm, GHOST_VOXEL, GHOST_TRUNC, 16, carve_voxels=carve)
    _clean(st0), _clean(st1)
    print(f"updates a point: {st0['n_updates'] / st0['n_points']:.2f} at C = 0, {st1['n_updates'] / st1['n_points']:.2f} at C = {carve}")
    check_ghost(e0, e1)


# ---- the weight scene: one wall, measured well from 4 m and badly from 16 m ----------------------------------------------------------
def weight_scene():
    """A wall at world z = 20.  From z = 16 it is 4 m away: d16 = 1550 measures 4.0004 m.  From z = 4 it is 16 m away, d16 = 388;
    raised by 8 (half a pixel of stereo error) it measures 15.658 m: 19.658 in the world."""
    prm = Param.default(base=0.5371, f=721.5377, cu=63.5, cv=3.5)

    def pose(z):
        T = np.eye(4)
        T[2, 3] = z
        return T
    near = (np.full((8, 128), 1550, np.int16), pose(16.0))
    far = (np.full((8, 128), 388 + 8, np.int16), pose(4.0))
    return prm, near, far


def shared_crossings_z(prm, near, far, fuse, **o):
    """z of the axis-2 crossings between voxels that both frames updated; fuse(frames, **o) gives the entries."""
    both = set(R.keys_of(fuse([near])["k"]).tolist()) & set(R.keys_of(fuse([far])["k"]).tolist())
    c = R.crossings(fuse([near, far], **o))
    c = c[c["axis"] == 2]
    kb = c["k"].astype(np.int64)
    kb[:, 2] += 1
    sel = np.array([a in both and b in both for a, b in zip(R.keys_of(c["k"]).tolist(), R.keys_of(kb).tolist())], bool)
    return R.crossing_points(c[sel], 0.2)[:, 2].astype(np.float64)


def check_weight_scene(prm, zu, zw):
    truth = prm.f * prm.base / (1550 / 16.0) + 16.0          # what the near view measures: 20.0004
    print(f"uniform: {len(zu)} crossings at {zu.min():.4f} .. {zu.max():.4f}; weighted: {len(zw)} at {zw.min():.4f} .. {zw.max():.4f}; near view {truth:.4f}")
    assert len(zu) > 0 and len(zw) > 0
    assert np.abs(zw - truth).max() < np.abs(zu - truth).min()


def test_weight_scene():
    prm, near, far = weight_scene()
    assert (CR.weight_of(1550, 12, 255), CR.weight_of(396, 12, 255)) == (255, 38)

    def fuse(frames, **o):
        e, st = CR.fuse(frames, prm, **o)
        _clean(st)
        return e
    check_weight_scene(prm, shared_crossings_z(prm, near, far, fuse), shared_crossings_z(prm, near, far, fuse, weight_shift=12, weight_max=255))


# ---- algebra -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("o", OPTIONS[1:])
def test_additivity_and_order(o):
    rng = np.random.default_rng(5)
    prm = _param()
    poses = [None, np.eye(4), POSE, POSE @ POSE, np.linalg.inv(POSE)]
    frames = [(random_map(rng, 9, 31, spread=1500, invalid=0.3), p) for p in poses]
    whole, st = CR.fuse(frames, prm, 0.2, 3, 16, **o)
    _clean(st)
    assert len(R.crossings(whole)) > 0
    assert _same(CR.fuse(frames[::-1], prm, 0.2, 3, 16, **o)[0], whole)
    for cut in (1, 2, 4):
        a, b = CR.fuse(frames[:cut], prm, 0.2, 3, 16, **o)[0], CR.fuse(frames[cut:], prm, 0.2, 3, 16, **o)[0]
        assert _same(R.merge(a, b), whole) and _same(R.merge(b, a), whole)
    parts = [CR.fuse([fr], prm, 0.2, 3, 16, **o)[0] for fr in frames]
    assert _same(R.merge(*parts), whole) and _same(R.merge(*parts[::-1]), whole)
    assert not _same(whole, R.fuse(frames, prm, 0.2, 3, 16)[0])


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
def test_option_defaults_and_the_prototypes():
    """The options are four scalars of viso_tsdf_set_fuse_options: there is no struct to lay out.  Their order and types in the
    prototype table, and the defaults' dict in that order."""
    assert list(TSDF_FUSE_DEFAULTS.items()) == [("carve_voxels", 0), ("weight_shift", -1), ("weight_max", 255), ("carve_near", 0.0)]
    assert PROTOTYPES["tsdf_set_fuse_options"] == (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_double])
    assert PROTOTYPES["tsdf_get_fuse_options"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                                             C.POINTER(C.c_double)])
    assert libviso_amd.tsdf_fuse_options() == TSDF_FUSE_DEFAULTS
    assert libviso_amd.tsdf_fuse_options(carve_voxels=28, weight_shift=12) == dict(carve_voxels=28, weight_shift=12, weight_max=255, carve_near=0.0)
    assert libviso_amd.tsdf_fuse_options(weight_shift=None)["weight_shift"] == -1
    with pytest.raises(TypeError):
        libviso_amd.tsdf_fuse_options(foo=1)
    assert isinstance(libviso_amd.TsdfMap.fuse_options, property)


BAD_OPTIONS = (dict(carve_voxels=-1), dict(carve_voxels=1025), dict(weight_shift=-2), dict(weight_shift=31), dict(weight_shift=0, weight_max=0),
               dict(weight_shift=12, weight_max=256), dict(carve_near=-0.5), dict(carve_near=float("nan")), dict(carve_near=float("inf")))


def _set(L, handle, **o):
    o = libviso_amd.tsdf_fuse_options(**o)
    return L.viso_tsdf_set_fuse_options(handle, o["carve_voxels"], o["weight_shift"], o["weight_max"], o["carve_near"])


def test_argument_errors_without_a_device():
    """The values are checked before the handle, so every refusal of a value is reached with a handle that is not a map; a handle
    that is not a map is refused without being followed."""
    L = libviso_amd.load()
    c, s, m, n = C.c_int32(1), C.c_int32(2), C.c_uint32(3), C.c_double(5.0)
    for handle in (None, C.c_void_p(4096)):
        for bad in BAD_OPTIONS:
            assert _set(L, handle, **bad) == -1, bad
            assert b"viso_tsdf_set_fuse_options: bad argument" in L.viso_last_error(), bad
        # values in range, the ends of the ranges among them; weight_max is read only with weights on, so 0 passes there: the
        # handle is refused next
        for ok in (dict(carve_voxels=1024, weight_shift=30, weight_max=1, carve_near=1e300), dict(weight_max=0), dict(weight_max=256), {},
                   dict(weight_shift=0, weight_max=255)):
            assert _set(L, handle, **ok) == -1
            assert b"viso_tsdf_set_fuse_options: not a live TSDF handle" in L.viso_last_error(), ok
        assert L.viso_tsdf_get_fuse_options(handle, C.byref(c), C.byref(s), C.byref(m), C.byref(n)) == -1
        assert b"viso_tsdf_get_fuse_options: not a live TSDF handle" in L.viso_last_error()
        assert L.viso_tsdf_get_fuse_options(handle, None, None, None, None) == -1
    assert (c.value, s.value, m.value, n.value) == (1, 2, 3, 5.0)   # nothing written
    with pytest.raises(TypeError):
        libviso_amd.TsdfMap(carve_voxels=3, foo=1)


def test_extended_kernels_have_no_scratch():
    res = kernel_resources("tsdf.hip", ("tsdf_carve_fuse_kernel", "tsdf_gray_carve_fuse_kernel"))
    for name, (occ, scratch) in res.items():
        print(f"{name}: occupancy {occ}, scratch {scratch}")
        assert scratch == 0 and occ >= 1
