"""The photometric frame-to-model alignment (include/viso_hip.h, "TSDF photometric align") without a device: the two restatements
of the linearise (tests/photo_align_ref.py) against each other and against the plain one (tests/align_ref.py), the intensity's
gradient against differences, the structs, the refusals that touch no device, the kernel's resource usage and the accuracy on the
textured scenes of tests/photo_align_cases.py.

Measured with the committed restatement (120 x 200, f 180, base 2.16, T = 3, three fused views; the fourth view aligned from a guess
0.448 degrees and 0.0838 m off; lambda 1/32, no photometric gate):
  wall, voxel 0.1, gate 2: plain status 2, 0.12811 degrees / 0.059176 m; photometric status 1 after 4 steps, 0.00181 / 0.000648
  wall, voxel 0.2, gate 1: plain status 2, 1.39267 degrees / 0.032406 m; photometric status 1 after 5 steps, 0.00923 / 0.000665
  room, voxel 0.1, gate 2: plain status 1, 0.02510 degrees / 0.001361 m; photometric status 1 after 4 steps, 0.01927 / 0.001398
  wall, voxel 0.1, from the true pose: 0.00181 degrees / 0.000647 m; with image noise of 3 gray levels: 0.00431 / 0.000772
Asserted: twice the measurement (DESIGN.md 5.19's factor, for its reason: discretisation noise that moves with the grid's phase)."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import libviso_amd
from libviso_amd import abi

import align_cases as AC
import align_ref as AR
import gray_ref as GR
import photo_align_cases as PC
import photo_align_ref as PR
import tsdf_tables as TT
from estimator_util import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = {("wall", 0.1): (0.00181, 0.000648), ("wall", 0.2): (0.00923, 0.000665)}    # degrees, metres
MEASURED_PLAIN_ROOM = (0.02510, 0.001361)                                               # tests/test_align_cpu.py's MEASURED


def _both(e, voxel, m, g, prm, pose, **kw):
    """The two restatements agree byte for byte; returns the vectorised result and the loop's trace."""
    trace = Counter()
    N, p, c = PR.linearize(e, voxel, m, g, prm, pose, **kw)
    Nl, pl, cl = PR.linearize_loop(e, voxel, m, g, prm, pose, trace=trace, **kw)
    assert N.dtype == np.int64 and N.tobytes() == Nl.tobytes() and p == pl and c == cl, (c, cl, p, pl)
    assert (N == N.T).all() and c["n_used"] == trace["used"] == trace["photo_used"] + trace["photo_gated"] + trace["photo_clipped"]
    assert c["n_photo_used"] == trace["photo_used"] and 0 <= p <= int(N[6, 6])
    return (N, p, c), trace


@pytest.mark.parametrize("shape", [(3, 130), (1, 1), (37, 333)])
@pytest.mark.parametrize("scene", ["wall", "room"])
def test_the_two_restatements_agree(shape, scene):
    prm = AC.wide_param(shape)
    m, g = PC.raycast(AC.FUSED[1], scene, shape, prm)
    e = PC.model(scene, 0.1)
    for pose in (AC.FUSED[1], AC.perturbed(AC.FUSED[1])):
        (N, p, c), trace = _both(e, 0.1, m, g, prm, pose, gate_voxels=2.0)
        assert c["n_photo_used"] > 0 and p > 0 and sum(trace[k] for k in AR.RULES) == m.size
        # the geometric part is the plain one: with lambda = 0 the second row is zero
        N0, p0, c0 = PR.linearize(e, 0.1, m, g, prm, pose, gate_voxels=2.0, photo_weight=0.0)
        Np, cp = AR.linearize(GR.plain(e), 0.1, m, prm, pose, gate_voxels=2.0)
        assert N0.tobytes() == Np.tobytes() and p0 == 0 and {k: c0[k] for k in AR.COUNTERS} == cp == {k: c[k] for k in AR.COUNTERS}
        assert c0["n_photo_used"] == c["n_photo_used"] == c["n_used"]


def test_the_two_restatements_agree_on_every_rule():
    """The rules of "TSDF align" on a random block with random intensities, then P3 (a gate of ten gray levels on the wall, seen from the guess) and P5
    (tests/photo_align_cases.py's clip_case), each with pixels that the rule ends and pixels that it does not."""
    e, m = PC.random_gray(AC.block()), AC.block_map()
    g = np.random.default_rng(8).integers(0, 256, m.shape).astype(np.uint8)
    for pose in (None, AC.perturbed(np.eye(4))):
        _, trace = _both(e, 0.2, m, g, AC.BLOCK_PARAM, pose, min_weight=1, photo_gate=60.0)
        assert all(trace[k] > 0 for k in ("invalid", "missing", "gated", "used", "photo_gated", "photo_used")), dict(trace)
    m, g = PC.frame("wall")
    (_, _, c), trace = _both(PC.model("wall", 0.1), 0.1, m[40:50], g[40:50], AC.param(), AC.GUESS, gate_voxels=2.0, photo_gate=10.0)
    assert trace["photo_gated"] > 100 and trace["photo_used"] > 100 and c["n_photo_gated"] == trace["photo_gated"], dict(trace)
    e, voxel, m, g, prm = PC.clip_case()
    (N, p, c), trace = _both(e, voxel, m, g, prm, None)
    assert trace["photo_clipped"] > 100 and trace["photo_used"] > 100 and c["n_photo_clipped"] == trace["photo_clipped"], dict(trace)
    assert c["n_clipped"] == 0 and p == int(N[6, 6]) == 80 * 80 * c["n_photo_used"] and not N[:6].any()    # r = 10: B_6 = 80
    e, voxel, m, g, prm = PC.one_run_case()
    (_, _, c), _ = _both(e, voxel, m, g, prm, None)
    assert c["n_photo_used"] == c["n_used"] == 128


def test_a_constant_image_on_a_constant_map_has_no_residual():
    m, _ = PC.frame("wall")
    e = PC.constant_gray(PC.model("wall", 0.2), 77)
    g = np.full(m.shape, 77, np.uint8)
    (N, p, c), _ = _both(e, 0.2, m[:6], g[:6], AC.param(), AC.GUESS)
    Np, _ = AR.linearize(GR.plain(e), 0.2, m[:6], AC.param(), AC.GUESS)
    assert c["n_photo_used"] == c["n_used"] > 500 and p == 0 and N.tobytes() == Np.tobytes()


def test_intensity_gradient_against_central_differences():
    """mu of P2 is multilinear in t: inside one cell its central difference is E up to rounding."""
    rng = np.random.default_rng(5)
    for _ in range(50):
        i = rng.uniform(0, 255, (2, 2, 2)).tolist()
        t = rng.uniform(0.05, 0.95, 3)
        mu, E = PR.interpolate(i, t)
        assert (mu, E) == AR.trilinear(i, t)
        for ax in range(3):
            lo, hi = t.copy(), t.copy()
            lo[ax] -= 0.03
            hi[ax] += 0.03
            diff = (PR.interpolate(i, hi)[0] - PR.interpolate(i, lo)[0]) / 0.06
            assert abs(diff - E[ax]) <= 1e-9 * 255, (ax, diff, E[ax])
        assert 0 <= mu <= 255


def test_struct_sizes_and_offsets(tmp_path):
    fields = {"viso_tsdf_align_gray_params": ("geo", "photo_weight", "photo_gate"),
              "viso_tsdf_normal_gray": ("normal.n",) + tuple("normal." + n for n in AR.COUNTERS) + ("p",) + PR.PHOTO_COUNTERS,
              "viso_tsdf_alignment_gray": ("a.pose", "a.cov", "a.cost", "a.n_used", "a.iters", "a.status", "cost_geo", "cost_photo", "n_photo_used"),
              "viso_tsdf_align_gray_step": ("pose", "normal")}
    src = ['#include <stdio.h>', '#include "viso_hip.h"', "int main(void) {"]
    for s, names in fields.items():
        src.append(f'printf("{s} %zu", sizeof({s}));')
        src += [f'printf(" %zu", offsetof({s}, {n}));' for n in names]
        src.append('printf("\\n");')
    src.append("return 0; }")
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    P = abi.TsdfAlignGrayParams
    assert got["viso_tsdf_align_gray_params"] == [C.sizeof(P)] + [getattr(P, n).offset for n in fields["viso_tsdf_align_gray_params"]] == [64, 0, 48, 56]
    for s, dt in (("viso_tsdf_normal_gray", abi.TSDF_NORMAL_GRAY_DTYPE), ("viso_tsdf_alignment_gray", abi.TSDF_ALIGNMENT_GRAY_DTYPE),
                  ("viso_tsdf_align_gray_step", abi.TSDF_ALIGN_GRAY_STEP_DTYPE)):
        assert got[s] == [dt.itemsize] + [dt.fields[n.split(".")[-1]][1] for n in fields[s]], s
    assert [got[s][0] for s in ("viso_tsdf_normal_gray", "viso_tsdf_alignment_gray", "viso_tsdf_align_gray_step")] == [304, 464, 432]
    # the plain structs lead the gray ones field for field
    for plain, gray in ((abi.TSDF_NORMAL_DTYPE, abi.TSDF_NORMAL_GRAY_DTYPE), (abi.TSDF_ALIGNMENT_DTYPE, abi.TSDF_ALIGNMENT_GRAY_DTYPE)):
        assert all(gray.fields[n][:2] == plain.fields[n][:2] for n in plain.names) and gray.names[:len(plain.names)] == plain.names
    p = libviso_amd.tsdf_align_gray_params()
    assert p.ok() and {k: getattr(p, k) for k in abi.TSDF_ALIGN_GRAY_DEFAULTS} == PR.PHOTO_DEFAULTS == abi.TSDF_ALIGN_GRAY_DEFAULTS
    assert {k: getattr(p.geo, k) for k in abi.TSDF_ALIGN_DEFAULTS} == abi.TSDF_ALIGN_DEFAULTS
    q = libviso_amd.tsdf_align_gray_params(gate_voxels=2.0, photo_gate=30)
    assert (q.geo.gate_voxels, q.photo_gate, q.photo_weight) == (2.0, 30.0, 1.0 / 32.0)
    with pytest.raises(TypeError):
        libviso_amd.tsdf_align_gray_params(photo=1.0)
    with pytest.raises(TypeError):
        libviso_amd.tsdf_align_params(photo_weight=1.0)


def test_symbols_are_declared_and_exported():
    L = libviso_amd.load()
    assert len(L.viso_tsdf_linearize_gray.argtypes) == 9 and len(L.viso_tsdf_align_gray.argtypes) == 11
    assert len(L.viso_batch_align_tsdf_gray.argtypes) == 7
    q = abi.TsdfAlignGrayParams()
    L.viso_tsdf_align_gray_params_default(C.byref(q))
    assert bytes(q) == bytes(libviso_amd.tsdf_align_gray_params())
    L.viso_tsdf_align_gray_params_default(None)


def test_argument_errors_with_any_handle():
    """What does not need the map is checked before the handle: VISO_ERR_ARG and "bad argument" whatever the handle is."""
    L = libviso_amd.load()
    prm = TT.param()
    d, img = np.full((2, 3), 300, np.int16), np.full((2, 3), 9, np.uint8)
    out, rec = np.zeros(1, abi.TSDF_NORMAL_GRAY_DTYPE), np.zeros(1, abi.TSDF_ALIGNMENT_GRAY_DTYPE)
    steps = np.zeros(3, abi.TSDF_ALIGN_GRAY_STEP_DTYPE)
    T = np.eye(4)
    dp, ip, Tp = d.ctypes.data_as(C.POINTER(C.c_int16)), img.ctypes.data_as(C.POINTER(C.c_uint8)), T.ctypes.data_as(C.POINTER(C.c_double))

    def params(**kw):
        p = libviso_amd.tsdf_align_gray_params()
        for k, v in kw.items():
            setattr(p.geo if k in abi.TSDF_ALIGN_DEFAULTS else p, k, v)
        return C.byref(p)

    def bad_param(**kw):
        p = TT.param()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def linearize(handle, p=None, disp=dp, image=ip, rows=2, cols=3, param=prm, pose=Tp, o=out.ctypes.data):
        return L.viso_tsdf_linearize_gray(handle, params() if p is None else p, disp, image, rows, cols,
                                          C.byref(param) if param is not None else None, pose, o)

    def align(handle, p=None, disp=dp, image=ip, rows=2, cols=3, param=prm, pose=Tp, o=rec.ctypes.data, trace=steps.ctypes.data, cap=3):
        return L.viso_tsdf_align_gray(handle, params() if p is None else p, disp, image, rows, cols,
                                      C.byref(param) if param is not None else None, pose, o, trace, cap)

    Tbad = T.copy()
    Tbad[1, 3] = np.nan
    wrong = [dict(p=C.POINTER(abi.TsdfAlignGrayParams)()), dict(image=None), dict(p=params(photo_weight=-1e-9)), dict(p=params(photo_weight=np.inf)),
             dict(p=params(photo_weight=np.nan)), dict(p=params(photo_gate=0.0)), dict(p=params(photo_gate=-3.0)), dict(p=params(photo_gate=np.inf)),
             dict(p=params(photo_gate=np.nan)), dict(p=params(min_weight=0)), dict(p=params(gate_voxels=0.0)), dict(p=params(max_iters=51)),
             dict(p=params(eps_rot=np.nan)), dict(p=params(min_pixels=5)), dict(disp=None), dict(param=None), dict(o=None), dict(rows=0),
             dict(cols=-1), dict(rows=2048, cols=2049), dict(pose=Tbad.ctypes.data_as(C.POINTER(C.c_double))), dict(param=bad_param(f=0.0)),
             dict(param=bad_param(base=np.nan))]
    for handle in (None, C.c_void_p(4096)):
        for name, call in (("viso_tsdf_linearize_gray", linearize), ("viso_tsdf_align_gray", align)):
            for kw in wrong:
                assert call(handle, **kw) == -1, (name, kw)
                msg = L.viso_last_error()
                assert name.encode() in msg and b"bad argument" in msg, (name, kw, msg)
            assert call(handle) == -1 and (name + ": not a live TSDF handle").encode() in L.viso_last_error()
            assert call(handle, p=params(photo_weight=0.0), pose=None) == -1 and b"not a live" in L.viso_last_error()
        assert align(handle, cap=-1) == -1 and b"bad argument" in L.viso_last_error()
        assert align(handle, trace=None, cap=2) == -1 and b"bad argument" in L.viso_last_error()
        assert L.viso_batch_align_tsdf_gray(handle, handle, 0, 1, Tp, params(), rec.ctypes.data) == -1
        assert L.viso_batch_align_tsdf_gray(handle, handle, 0, 1, Tp, None, rec.ctypes.data) == -1 and b"bad argument" in L.viso_last_error()
    assert not out.tobytes().strip(b"\0") and not rec.tobytes().strip(b"\0") and not steps.tobytes().strip(b"\0")
    # the wrapper: an image goes with a gray map only, and has the map's shape and type
    for gray, bad in ((False, img), (True, img[:1]), (True, img.astype(np.int8))):
        m = object.__new__(libviso_amd.TsdfMap)
        m.L, m.h, m.gray = L, 4096, gray
        try:
            with pytest.raises(ValueError):
                m.linearize(d, prm, image=bad)
            with pytest.raises(ValueError):
                m.align(d, prm, image=bad, trace=True)
            if gray:
                with pytest.raises(libviso_amd.VisoError, match="-1"):
                    m.linearize(d, prm, image=img)
                with pytest.raises(TypeError):
                    m.align(d, prm, image=img, photo=2.0)
                with pytest.raises(TypeError):
                    m.align(d, prm, photo_weight=2.0)       # without an image: the plain call, which has no such parameter
        finally:
            m.h = None


def test_gray_linearize_kernel_has_no_scratch_and_the_plain_one_keeps_its_occupancy():
    res = kernel_resources("tsdf_align.hip", ("tsdf_linearize_kernel", "tsdf_gray_linearize_kernel"))
    print(res)
    assert res["tsdf_gray_linearize_kernel"][1] == 0 and res["tsdf_gray_linearize_kernel"][0] >= 2
    assert res["tsdf_linearize_kernel"] == (4, 0)


def _run(scene, voxel, gate, guess=None, **kw):
    e, (m, g) = PC.model(scene, voxel), PC.frame(scene)
    rec, steps = PR.align(e, voxel, m, g, AC.param(), AC.GUESS if guess is None else guess, gate_voxels=gate, **kw)
    return rec, steps, AR.pose_error(rec["pose"], AC.TRUTH)


@pytest.mark.parametrize("voxel,gate", [(0.1, 2.0), (0.2, 1.0)])
def test_the_wall_is_held_by_its_texture(voxel, gate):
    """One plane: the plain alignment leaves the in-plane motion where the guess put it and reports no failure; the photometric
    one converges to the truth."""
    prm, e, (m, g) = AC.param(), PC.model("wall", voxel), PC.frame("wall")
    guess_err = AR.pose_error(AC.GUESS, AC.TRUTH)
    plain, _ = AR.align(GR.plain(e), voxel, m, prm, AC.GUESS, gate_voxels=gate)
    plain_err = AR.pose_error(plain["pose"], AC.TRUTH)
    print(f"plain: status {plain['status']}, error {plain_err[0]:.5f} degrees {plain_err[1]:.6f} m (guess {guess_err[0]:.3f} {guess_err[1]:.4f})")
    # the condition: plain reports no failure and does not hold the wall (at 0.2 its rotation ends worse than the guess's)
    assert plain["status"] > 0 and (plain_err[1] > 0.5 * guess_err[1] if voxel == 0.1 else plain_err[0] > guess_err[0])
    rec, steps, err = _run("wall", voxel, gate)
    print(f"photometric: status {rec['status']}, {rec['iters']} steps, {rec['n_photo_used']} of {rec['n_used']} rows, cost {rec['cost_geo']:.4f} px "
          f"{rec['cost_photo']:.3f} gray levels, error {err[0]:.5f} degrees {err[1]:.6f} m")
    assert rec["status"] == 1 and rec["iters"] <= 6 and len(steps) == rec["iters"] + 1
    assert err[0] <= 2 * MEASURED["wall", voxel][0] and err[1] <= 2 * MEASURED["wall", voxel][1]
    assert err[1] < 0.1 * plain_err[1]
    assert rec["n_photo_used"] == rec["n_used"] > m.size // 2 and 0 < rec["cost_geo"] < rec["cost"] and 0 < rec["cost_photo"] < 8
    cov = rec["cov"]
    assert np.allclose(cov, cov.T, rtol=1e-9, atol=0) and (np.linalg.eigvalsh((cov + cov.T) / 2) > 0).all()
    # the loop restatement walks the same trajectory
    if voxel == 0.2:
        rec_l, steps_l = PR.align(e, voxel, m[::4], g[::4], prm, AC.GUESS, gate_voxels=gate, max_iters=2, loop=True)
        rec_v, steps_v = PR.align(e, voxel, m[::4], g[::4], prm, AC.GUESS, gate_voxels=gate, max_iters=2)
        assert rec_l["pose"].tobytes() == rec_v["pose"].tobytes() and rec_l["cov"].tobytes() == rec_v["cov"].tobytes()
        assert [s[2] for s in steps_l] == [s[2] for s in steps_v]


def test_from_the_true_pose_the_wall_stays():
    rec, _, err = _run("wall", 0.1, 2.0, guess=AC.TRUTH)
    print(f"from the truth: status {rec['status']}, {rec['iters']} steps, error {err[0]:.5f} degrees {err[1]:.6f} m")
    assert rec["status"] == 1 and err[0] <= 2 * MEASURED["wall", 0.1][0] and err[1] <= 2 * MEASURED["wall", 0.1][1]


def test_the_room_is_not_harmed():
    rec, _, err = _run("room", 0.1, 2.0)
    print(f"room: status {rec['status']}, {rec['iters']} steps, error {err[0]:.5f} degrees {err[1]:.6f} m")
    assert rec["status"] == 1 and err[0] <= 2 * MEASURED_PLAIN_ROOM[0] and err[1] <= 2 * MEASURED_PLAIN_ROOM[1]


def test_failures_return_the_guess():
    m, g = PC.frame("wall")
    rec, steps = PR.align(PC.model("wall", 0.1), 0.1, m[:2, :90], g[:2, :90], AC.param(), AC.GUESS, gate_voxels=2.0)
    assert rec["status"] == -1 and len(steps) == 1 and (rec["pose"] == AC.GUESS).all()
    assert (rec["cost_geo"], rec["cost_photo"], rec["n_photo_used"], rec["n_used"]) == (0.0, 0.0, 0, 0)
    # an image without texture on a single wall: as degenerate as the plain alignment
    e = PC.constant_gray(PC.model("wall", 0.2), 50)
    rec, steps = PR.align(e, 0.2, m, np.full(m.shape, 50, np.uint8), AC.param(), AC.GUESS)
    plain, _ = AR.align(GR.plain(e), 0.2, m, AC.param(), AC.GUESS)
    assert rec["status"] == plain["status"] and rec["pose"].tobytes() == plain["pose"].tobytes()
