"""Which refusal wins, and its text, when a call on the map layer breaks two rules at once: the host-pointer calls of the voxel map
and the TSDF map (fuse, linearise, align) and the batch's four consumers of its resident maps.  The other tests of these calls match
the return code only; here viso_last_error() is compared whole, so an order that changes is seen.  Every expected text is read from
the C sources' order of checks, never from a run: a fuse asks its registry first and its arguments afterwards, an alignment checks
whatever needs no map before it asks for the handle, and a batch call checks the batch's side before the map's."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd import hostmath, synth
from libviso_amd.abi import TSDF_ALIGNMENT_DTYPE, TSDF_ALIGNMENT_GRAY_DTYPE, TSDF_NORMAL_DTYPE, TSDF_NORMAL_GRAY_DTYPE, MatchParams, Param

pytestmark = pytest.mark.gpu

ARG = -1
NOT_MAP, NOT_TSDF = "not a live map handle", "not a live TSDF handle"
FUSE_ARGS = "bad argument (non-null map and calibration, sizes > 0)"
FUSE_POSE = "a pose has an entry that is not finite"
NO_INTENSITY = "the TSDF map carries no intensity (viso_tsdf_create_gray makes one that does)"
HAS_INTENSITY = "the TSDF map carries intensity: its calls are the *_gray ones"
NO_IMAGE = "bad argument (a non-null image)"
LIN_ARGS = "bad argument (non-null map, calibration and output)"
ALIGN_ARGS = "bad argument (non-null map, calibration and record, trace_cap >= 0 and 0 without a trace)"
GRAY_ARGS = "bad argument (non-null parameters and image)"
CALIB = "bad argument (the calibration f, cu, cv, base must be finite, f > 0 and base > 0)"
GATE = "bad argument (gate_voxels 100 is beyond the map's truncation of 1 voxels)"
RANGE = "bad argument (live handles, 0 <= t0 < t1 <= n_frames, poses [t1 - t0][16])"
ALIGN_POSE = "bad argument (pose 1 has an entry that is not finite)"
NOT_READY = "dense disparity is off, or no run has computed it"

RES_SHAPE = (120, 400)


def _i16(a):
    return a.ctypes.data_as(C.POINTER(C.c_int16))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _f64(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _dead(make):
    """The handle of a map that has been destroyed."""
    t = make()
    h = t.h
    t.close()
    return h


def _overflowed(ctx, gray):
    """A TSDF map of 1024 slots that the existing 1 x 2000 map has overflowed (truncation: 1 voxel)."""
    wide, img = np.full((1, 2000), 16, np.int16), np.full((1, 2000), 7, np.uint8)
    t = libviso_amd.TsdfMap(ctx, gray=gray, voxel=0.5, trunc_voxels=1, min_disp16=1, capacity_log2=10)
    with pytest.raises(libviso_amd.VisoError, match="-4"):
        t.fuse(wide, Param.default(base=1.0, f=2.0, cu=0.0, cv=0.0), **(dict(image=img) if gray else {}))
    return t


def _check(L, table):
    for entry, pair, call, text in table:
        r = call()
        got = L.viso_last_error().decode()
        print(f"{entry}: {pair}: {r} {got}")
        assert r == ARG and got == f"{entry}: {text}", (entry, pair, r, got)


def test_host_fuses(viso):
    L = viso
    m, img = np.full((4, 8), 16, np.int16), np.full((4, 8), 7, np.uint8)
    prm, inf = Param.default(base=1.0, f=2.0, cu=0.0, cv=0.0), Param.default(base=1.0, f=float("inf"), cu=0.0, cv=0.0)
    vmap = libviso_amd.VoxelMap(None, capacity_log2=10)
    plain, gray = libviso_amd.TsdfMap(None, capacity_log2=10), libviso_amd.TsdfMap(None, gray=True, capacity_log2=10)
    dead_map = _dead(lambda: libviso_amd.VoxelMap(None, capacity_log2=10))
    dead_tsdf = _dead(lambda: libviso_amd.TsdfMap(None, capacity_log2=10))
    P = C.byref
    _check(L, [
        # entry point, the two rules broken, the call, the text of the rule that wins
        ("viso_map_fuse", "dead handle | null map", lambda: L.viso_map_fuse(dead_map, None, 4, 8, P(prm), None), NOT_MAP),
        ("viso_map_fuse", "null map | non-finite calibration", lambda: L.viso_map_fuse(vmap.h, None, 4, 8, P(inf), None), FUSE_ARGS),
        ("viso_tsdf_fuse", "dead handle | null map", lambda: L.viso_tsdf_fuse(dead_tsdf, None, 4, 8, P(prm), None), NOT_TSDF),
        ("viso_tsdf_fuse", "null map | non-finite calibration", lambda: L.viso_tsdf_fuse(plain.h, None, 4, 8, P(inf), None), FUSE_ARGS),
        ("viso_tsdf_fuse", "wrong map kind | null map", lambda: L.viso_tsdf_fuse(gray.h, None, 4, 8, P(prm), None), HAS_INTENSITY),
        ("viso_tsdf_fuse_gray", "dead handle | missing image", lambda: L.viso_tsdf_fuse_gray(dead_tsdf, _i16(m), None, 4, 8, P(prm), None), NOT_TSDF),
        ("viso_tsdf_fuse_gray", "wrong map kind | missing image", lambda: L.viso_tsdf_fuse_gray(plain.h, _i16(m), None, 4, 8, P(prm), None), NO_INTENSITY),
        ("viso_tsdf_fuse_gray", "missing image | null map", lambda: L.viso_tsdf_fuse_gray(gray.h, None, None, 4, 8, P(prm), None), NO_IMAGE),
        ("viso_tsdf_fuse_gray", "null map | non-finite calibration", lambda: L.viso_tsdf_fuse_gray(gray.h, None, _u8(img), 4, 8, P(inf), None), FUSE_ARGS),
    ])
    assert vmap.count() == 0 and len(plain.entries()) == 0 and len(gray.entries(gray=True)) == 0
    for t in (vmap, plain, gray):
        t.close()


def test_host_alignments(viso):
    L = viso
    m, img = np.full((4, 8), 16, np.int16), np.full((4, 8), 7, np.uint8)
    prm, inf = Param.default(base=1.0, f=2.0, cu=0.0, cv=0.0), Param.default(base=1.0, f=float("inf"), cu=0.0, cv=0.0)
    plain = libviso_amd.TsdfMap(None, capacity_log2=10)
    dead = _dead(lambda: libviso_amd.TsdfMap(None, capacity_log2=10))
    full, full_gray = _overflowed(None, False), _overflowed(None, True)
    p, far = libviso_amd.tsdf_align_params(), libviso_amd.tsdf_align_params(gate_voxels=100.0)
    pg, far_g = libviso_amd.tsdf_align_gray_params(), libviso_amd.tsdf_align_gray_params(gate_voxels=100.0)
    out, rec = np.zeros(1, TSDF_NORMAL_DTYPE), np.zeros(1, TSDF_ALIGNMENT_DTYPE)
    out_g, rec_g = np.zeros(1, TSDF_NORMAL_GRAY_DTYPE), np.zeros(1, TSDF_ALIGNMENT_GRAY_DTYPE)
    o, r, og, rg = out.ctypes.data, rec.ctypes.data, out_g.ctypes.data, rec_g.ctypes.data
    P, M, I = C.byref, _i16(m), _u8(img)
    _check(L, [
        ("viso_tsdf_linearize", "dead handle | null map", lambda: L.viso_tsdf_linearize(dead, P(p), None, 4, 8, P(prm), None, o), LIN_ARGS),
        ("viso_tsdf_linearize", "dead handle | non-finite calibration", lambda: L.viso_tsdf_linearize(dead, P(p), M, 4, 8, P(inf), None, o), CALIB),
        ("viso_tsdf_linearize", "null map | non-finite calibration", lambda: L.viso_tsdf_linearize(plain.h, P(p), None, 4, 8, P(inf), None, o), LIN_ARGS),
        ("viso_tsdf_linearize", "gate beyond truncation | overflowed table", lambda: L.viso_tsdf_linearize(full.h, P(far), M, 4, 8, P(prm), None, o), GATE),
        ("viso_tsdf_align", "dead handle | null map", lambda: L.viso_tsdf_align(dead, P(p), None, 4, 8, P(prm), None, r, None, 0), ALIGN_ARGS),
        ("viso_tsdf_align", "dead handle | non-finite calibration", lambda: L.viso_tsdf_align(dead, P(p), M, 4, 8, P(inf), None, r, None, 0), CALIB),
        ("viso_tsdf_align", "null map | non-finite calibration", lambda: L.viso_tsdf_align(plain.h, P(p), None, 4, 8, P(inf), None, r, None, 0), ALIGN_ARGS),
        ("viso_tsdf_align", "gate beyond truncation | overflowed table", lambda: L.viso_tsdf_align(full.h, P(far), M, 4, 8, P(prm), None, r, None, 0), GATE),
        ("viso_tsdf_linearize_gray", "dead handle | null map", lambda: L.viso_tsdf_linearize_gray(dead, P(pg), None, I, 4, 8, P(prm), None, og), LIN_ARGS),
        ("viso_tsdf_linearize_gray", "null map | non-finite calibration", lambda: L.viso_tsdf_linearize_gray(full_gray.h, P(pg), None, I, 4, 8, P(inf), None, og), LIN_ARGS),
        ("viso_tsdf_linearize_gray", "wrong map kind | missing image", lambda: L.viso_tsdf_linearize_gray(plain.h, P(pg), M, None, 4, 8, P(prm), None, og), GRAY_ARGS),
        ("viso_tsdf_linearize_gray", "wrong map kind | gate beyond truncation", lambda: L.viso_tsdf_linearize_gray(full.h, P(far_g), M, I, 4, 8, P(prm), None, og), NO_INTENSITY),
        ("viso_tsdf_linearize_gray", "gate beyond truncation | overflowed table", lambda: L.viso_tsdf_linearize_gray(full_gray.h, P(far_g), M, I, 4, 8, P(prm), None, og), GATE),
        ("viso_tsdf_align_gray", "dead handle | null map", lambda: L.viso_tsdf_align_gray(dead, P(pg), None, I, 4, 8, P(prm), None, rg, None, 0), ALIGN_ARGS),
        ("viso_tsdf_align_gray", "null map | non-finite calibration", lambda: L.viso_tsdf_align_gray(full_gray.h, P(pg), None, I, 4, 8, P(inf), None, rg, None, 0), ALIGN_ARGS),
        ("viso_tsdf_align_gray", "wrong map kind | missing image", lambda: L.viso_tsdf_align_gray(plain.h, P(pg), M, None, 4, 8, P(prm), None, rg, None, 0), GRAY_ARGS),
        ("viso_tsdf_align_gray", "wrong map kind | gate beyond truncation", lambda: L.viso_tsdf_align_gray(full.h, P(far_g), M, I, 4, 8, P(prm), None, rg, None, 0), NO_INTENSITY),
        ("viso_tsdf_align_gray", "gate beyond truncation | overflowed table", lambda: L.viso_tsdf_align_gray(full_gray.h, P(far_g), M, I, 4, 8, P(prm), None, rg, None, 0), GATE),
    ])
    assert not any(a.tobytes().strip(b"\0") for a in (out, rec, out_g, rec_g))   # a refused call writes nothing
    for t in (plain, full, full_gray):
        t.close()


def test_batch_consumers(viso):
    L = viso
    prm = Param.default(base=0.5371, f=360.0, cu=199.5, cv=59.5)
    rng = np.random.default_rng(0)
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, 2, 64)
    b.upload_images_only(rng.integers(0, 256, (2, 2) + RES_SHAPE, dtype=np.uint8))
    b.set_params(MatchParams.stereo(hostmath.F_from_P(synth.KITTI_P1, synth.KITTI_P2)), MatchParams.temporal(), prm)
    b.set_disparity(num_disp=64)
    b.run_disparity()
    here_plain, full, full_gray = libviso_amd.TsdfMap(ctx, capacity_log2=10), _overflowed(ctx, False), _overflowed(ctx, True)
    # maps of another context (the default one)
    far_map = libviso_amd.VoxelMap(None, capacity_log2=10)
    far_plain, far_gray = libviso_amd.TsdfMap(None, capacity_log2=10), libviso_amd.TsdfMap(None, gray=True, capacity_log2=10)
    dead_map = _dead(lambda: libviso_amd.VoxelMap(ctx, capacity_log2=10))
    dead_tsdf = _dead(lambda: libviso_amd.TsdfMap(ctx, capacity_log2=10))
    eye = np.ascontiguousarray(np.tile(np.eye(4), (2, 1, 1)))
    bad = eye.copy(); bad[1, 0, 0] = np.inf
    E, B = _f64(eye), _f64(bad)
    p, far = libviso_amd.tsdf_align_params(), libviso_amd.tsdf_align_params(gate_voxels=100.0)
    pg, far_g = libviso_amd.tsdf_align_gray_params(), libviso_amd.tsdf_align_gray_params(gate_voxels=100.0)
    rec, rec_g = np.zeros(2, TSDF_ALIGNMENT_DTYPE), np.zeros(2, TSDF_ALIGNMENT_GRAY_DTYPE)
    r, rg = rec.ctypes.data, rec_g.ctypes.data
    P = C.byref
    fuse_d, fuse_t, align, align_g = "viso_batch_fuse_disparities", "viso_batch_fuse_tsdf", "viso_batch_align_tsdf", "viso_batch_align_tsdf_gray"
    _check(L, [
        (fuse_d, "dead handle | frames out of range", lambda: L.viso_batch_fuse_disparities(b.h, dead_map, -1, 1, E), RANGE),
        (fuse_d, "dead handle | non-finite pose", lambda: L.viso_batch_fuse_disparities(b.h, dead_map, 0, 2, B), NOT_MAP),
        (fuse_d, "non-finite pose | map of another context", lambda: L.viso_batch_fuse_disparities(b.h, far_map.h, 0, 2, B), FUSE_POSE),
        (fuse_t, "dead handle | frames out of range", lambda: L.viso_batch_fuse_tsdf(b.h, dead_tsdf, -1, 1, E), RANGE),
        (fuse_t, "dead handle | non-finite pose", lambda: L.viso_batch_fuse_tsdf(b.h, dead_tsdf, 0, 2, B), NOT_TSDF),
        (fuse_t, "non-finite pose | map of another context", lambda: L.viso_batch_fuse_tsdf(b.h, far_plain.h, 0, 2, B), FUSE_POSE),
        (fuse_t, "non-finite pose | gray map of another context", lambda: L.viso_batch_fuse_tsdf(b.h, far_gray.h, 0, 2, B), FUSE_POSE),
        (align, "dead handle | frames out of range", lambda: L.viso_batch_align_tsdf(b.h, dead_tsdf, -1, 1, E, P(p), r), RANGE),
        (align, "dead handle | non-finite pose", lambda: L.viso_batch_align_tsdf(b.h, dead_tsdf, 0, 2, B, P(p), r), ALIGN_POSE),
        (align, "non-finite pose | map of another context", lambda: L.viso_batch_align_tsdf(b.h, far_plain.h, 0, 2, B, P(p), r), ALIGN_POSE),
        (align, "gate beyond truncation | overflowed table", lambda: L.viso_batch_align_tsdf(b.h, full.h, 0, 2, E, P(far), r), GATE),
        (align_g, "dead handle | frames out of range", lambda: L.viso_batch_align_tsdf_gray(b.h, dead_tsdf, -1, 1, E, P(pg), rg), RANGE),
        (align_g, "non-finite pose | map of another context", lambda: L.viso_batch_align_tsdf_gray(b.h, far_gray.h, 0, 2, B, P(pg), rg), ALIGN_POSE),
        (align_g, "wrong map kind | gate beyond truncation", lambda: L.viso_batch_align_tsdf_gray(b.h, here_plain.h, 0, 2, E, P(far_g), rg), NO_INTENSITY),
        (align_g, "gate beyond truncation | overflowed table", lambda: L.viso_batch_align_tsdf_gray(b.h, full_gray.h, 0, 2, E, P(far_g), rg), GATE),
    ])
    # Resident images of another geometry: the upload that brings them drops the maps, so the batch's own refusal wins over the
    # map's kind, and "the resident images are not the maps'" is never the text.
    b.upload_images_only(rng.integers(0, 256, (2, 2, 60, 200), dtype=np.uint8))
    _check(L, [
        (align_g, "resident images of another geometry | plain map", lambda: L.viso_batch_align_tsdf_gray(b.h, here_plain.h, 0, 2, E, P(pg), rg), NOT_READY),
        (fuse_t, "resident images of another geometry | gray map of another context", lambda: L.viso_batch_fuse_tsdf(b.h, far_gray.h, 0, 2, E), NOT_READY),
    ])
    assert not rec.tobytes().strip(b"\0") and not rec_g.tobytes().strip(b"\0")
    assert far_map.count() == 0 and not any(len(t.entries()) for t in (far_plain, far_gray, here_plain))
    for t in (here_plain, full, full_gray, far_map, far_plain, far_gray):
        t.close()
    b.close(); ctx.close()
