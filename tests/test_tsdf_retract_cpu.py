"""The restatement of the TSDF retract (tests/retract_ref.py; include/viso_hip.h, "TSDF retract") held to its properties, with no
device: retracting a frame gives the map that never saw it, retracting every frame gives the empty map, the order of retracts does
not matter, and each refusal hands the map back untouched.  The scenes and option sets are the device tests' too
(tests/test_gpu_tsdf_retract.py imports them)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from libviso_amd import hostmath
from libviso_amd.abi import PROTOTYPES, Param, TsdfRetractReport

import evict_ref as E
import gray_ref as G
import retract_ref as RT
import tsdf_ref as R

INV = R.INVALID
# three distinct poses, close enough that the frames share voxels
POSES = [np.linalg.inv(hostmath.tr2mat(v)) for v in ([0.013, -0.021, 0.007, 0.31, -0.12, 1.47], [0.010, -0.017, 0.009, 0.36, -0.10, 1.39],
                                                     [0.016, -0.024, 0.004, 0.27, -0.15, 1.55])]
OPTIONS = {"default": {}, "carve": dict(carve_voxels=6), "weights": dict(weight_shift=12, weight_max=255),
           "both": dict(carve_voxels=6, weight_shift=12, weight_max=255)}
SHAPES = [(1, 1), (3, 130), (37, 333)]
VOXEL, TRUNC, MIN_DISP16 = 0.2, 3, 16


def param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)   # non-integer cu, cv


def mixed_map(rng, rows, cols, invalid=0.25):
    """tests/test_gpu_tsdf_carve.py's _mixed_map: patches of equal disparity seven pixels wide, broken up by single pixels and
    invalid ones, so that the runs inside a wave have many lengths and, with weights, lanes of one run carry different w."""
    m = np.repeat(rng.integers(16, 90 * 16 + 1, (rows, cols // 7 + 1)), 7, axis=1)[:, :cols]
    single = rng.random((rows, cols)) < 0.3
    m = np.where(single, rng.integers(16, 90 * 16 + 1, (rows, cols)), m).astype(np.int16)
    m[rng.random((rows, cols)) < invalid] = INV
    return m


def scene(shape, gray, seed=0):
    """The frames A, B, C of a case: (map, pose), with gray (map, image, pose).  B and C are A with a third of the pixels drawn
    again, so the three share many voxels and each has voxels of its own."""
    rng = np.random.default_rng(shape[0] * 3 + shape[1] + seed)
    if shape == (1, 1):
        maps = [np.array([[v]], np.int16) for v in (400, 400, 417)]
    else:
        a = mixed_map(rng, *shape)
        a[0, 60:70] = 200                # one run across the first wave boundary
        a.flat[0], a.flat[-1] = 0, 15    # below min_disp16
        maps = [a]
        for _ in range(2):
            other = mixed_map(rng, *shape)
            maps.append(np.where(rng.random(shape) < 0.33, other, a).astype(np.int16))
    images = [rng.integers(0, 256, shape).astype(np.uint8) for _ in maps]
    return [(m, im, T) if gray else (m, T) for m, im, T in zip(maps, images, POSES)]


def fuse(frames, gray, o, voxel=VOXEL):
    """The restatement's map of `frames`: input condition of every case: nothing out of range, nothing dropped (no weight wraps:
    carve_ref asserts it)."""
    e, st = RT.fuse(frames, param(), voxel, TRUNC, MIN_DISP16, gray=gray, **o)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0, st
    return e, st


def retract(e, st, frames, gray, o, voxel=VOXEL):
    return RT.retract(e, st, frames, param(), voxel, TRUNC, MIN_DISP16, gray=gray, **o)


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("options", sorted(OPTIONS))
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_retract_gives_the_map_that_never_saw_the_frame(shape, gray, options):
    o = OPTIONS[options]
    A, B, C_ = scene(shape, gray)
    e, st = fuse([A, B, C_], gray, o)
    want, wst = fuse([A, C_], gray, o)
    alone, ast = fuse([B], gray, o)
    got, gst, rep, ok = retract(e, st, [B], gray, o)
    assert ok and same(got, want) and gst == wst
    assert rep == dict(n_points=ast["n_points"], n_updates=ast["n_updates"], n_missing=0, n_underflow=0, n_inconsistent=0,
                       n_freed=len(e) - len(want))
    if shape != (1, 1):
        # the frames share voxels and B has voxels of its own: both halves of the call are in play
        assert rep["n_freed"] > 0 and len(alone) > rep["n_freed"]
    if gray:
        assert (got["gray"] <= 255 * got["weight"].astype(np.uint64)).all()


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_to_empty_in_any_order(shape, gray):
    o = OPTIONS["both"]
    frames = scene(shape, gray)
    e, st = fuse(frames, gray, o)
    got, gst, rep, ok = retract(e, st, frames, gray, o)                       # all in one call
    assert ok and len(got) == 0 and gst == dict(n_points=0, n_updates=0, n_out_of_range=0, n_occupied=0, n_dropped=0)
    assert rep["n_freed"] == len(e) and rep["n_updates"] == st["n_updates"]
    results = []
    for order in ((2, 0, 1), (1, 2, 0)):                                        # one by one
        cur, cst, freed = e, st, 0
        for i, k in enumerate(order):
            cur, cst, rep, ok = retract(cur, cst, [frames[k]], gray, o)
            assert ok
            freed += rep["n_freed"]
            if i == 0:
                results.append((cur, cst))
                assert same(cur, fuse([frames[j] for j in range(3) if j != k], gray, o)[0])
        assert len(cur) == 0 and cst["n_occupied"] == 0 and cst["n_updates"] == 0 and freed == len(e)
    # retracting two frames in either order leaves the third
    for first, second, left in ((0, 1, 2), (1, 0, 2)):
        cur, cst, _, ok1 = retract(e, st, [frames[first]], gray, o)
        cur, cst, _, ok2 = retract(cur, cst, [frames[second]], gray, o)
        want, wst = fuse([frames[left]], gray, o)
        assert ok1 and ok2 and same(cur, want) and cst == wst


def _refused(e, st, frames, gray, o, causes, voxel=VOXEL):
    """The call is refused for one of `causes` and hands back the very arrays it was given."""
    got, gst, rep, ok = retract(e, st, frames, gray, o, voxel)
    assert not ok and got is e and gst is st, rep
    assert any(rep[c] for c in causes), (causes, rep)
    return rep


def refusal_cases(gray):
    """(name, the fused frames, their options, the retracted frame, its options, the report's fields of which one names the cause) of
    every refusal that needs no eviction: shared with the device tests."""
    shape = (37, 333)
    A, B, C_ = scene(shape, gray)
    far = np.linalg.inv(hostmath.tr2mat([0.0, 0.0, 0.0, 500.0, 0.0, 0.0]))
    never = scene(shape, gray, seed=5)[1]
    cases = [("never fused, far away", [A, B, C_], {}, never[:-1] + (far,), {}, ("n_missing",)),
             ("B at A's pose", [A, B, C_], {}, B[:-1] + (A[-1],), {}, ("n_missing", "n_underflow", "n_inconsistent")),
             ("other options: carved", [A, B, C_], {}, B, OPTIONS["carve"], ("n_missing", "n_underflow", "n_inconsistent")),
             # (the other way round, fused with weights and retracted without, is one of the wrong calls that pass: every voxel
             # keeps a weight and a sum that its remaining updates could have left)
             ("other options: weighted", [A, B, C_], {}, B, OPTIONS["weights"], ("n_underflow", "n_inconsistent"))]
    if gray:
        dark = (B[0], np.zeros(shape, np.uint8), B[2])
        bright = (B[0], np.full(shape, 255, np.uint8), B[2])
        cases.append(("another image", [A, dark, C_], {}, bright, {}, ("n_inconsistent", "n_underflow")))
    return cases


@pytest.mark.parametrize("gray", [False, True])
def test_refusals_leave_the_map_untouched(gray):
    for name, frames, o, frame, ro, causes in refusal_cases(gray):
        e, st = fuse(frames, gray, o)
        rep = _refused(e, st, [frame], gray, ro, causes)
        if name == "never fused, far away":
            assert rep["n_missing"] == rep["n_updates"] > 0 and rep["n_freed"] == 0
    # B twice
    A, B, C_ = scene((37, 333), gray)
    e, st = fuse([A, B, C_], gray, {})
    once, ost, _, ok = retract(e, st, [B], gray, {})
    assert ok
    rep = _refused(once, ost, [B], gray, {}, ("n_missing", "n_underflow"))
    assert rep["n_missing"] > 0                                               # B's own voxels have left the table
    # B after an eviction that removed part of it
    lo, hi = E.box_around(POSES[1][:3, 3] + POSES[1][:3, :3] @ np.array([0.0, 0.0, 12.0]), 6.0, VOXEL)
    kept, gone = E.split(e, lo, hi)
    assert len(gone) and len(kept)
    rep = _refused(kept, dict(st, n_occupied=len(kept)), [B], gray, {}, ("n_missing",))
    # ... and from the map rebuilt from the archive it is retracted
    merge = G.merge if gray else R.merge
    got, _, _, ok = retract(merge(kept, gone), st, [B], gray, {})
    assert ok and same(got, fuse([A, C_], gray, {})[0])


def test_a_frame_that_was_never_fused_can_pass():
    """What the checks cannot see: updates that all land on voxels of the table and leave them within their bounds."""
    A, B, _ = scene((3, 130), False)
    e, st = fuse([A, A, A, B], False, {})
    impostor = (A[0].copy(), A[1])
    impostor[0][impostor[0] == 200] = INV                                      # A without its long run: never fused as such
    got, gst, rep, ok = retract(e, st, [impostor], False, {})
    assert ok and rep["n_updates"] > 0 and not same(got, fuse([A, A, B], False, {})[0])


def test_report_struct_is_the_header_s():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "viso_hip.h")).read()
    order = sorted(re.findall(r"#define VISO_RETRACT_(\w+) (\d)", hdr), key=lambda m: int(m[1]))
    assert [n.lower() for n, _ in order] == [n for n, _ in TsdfRetractReport._fields_] == list(RT.REPORT)
    assert [int(i) for _, i in order] == list(range(6)) and C.sizeof(TsdfRetractReport) == 48
    rep = TsdfRetractReport(*range(1, 7))
    assert [rep.words()[i] for i in range(6)] == list(range(1, 7)) and rep.as_dict()["n_freed"] == 6
    for name in ("tsdf_retract", "tsdf_retract_gray", "batch_retract_tsdf", "tsdf_move", "tsdf_move_gray", "batch_move_tsdf"):
        assert PROTOTYPES[name][1][-1] == C.POINTER(C.c_uint64)
