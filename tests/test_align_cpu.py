"""The frame-to-model alignment (include/viso_hip.h, "TSDF align") without a device: the two numpy restatements of the linearise
(tests/align_ref.py) against each other, the analytic gradient against differences, the loop on the analytic scene of
tests/align_cases.py, the structs, the refusals of the C ABI that touch no device and the kernel's resource usage.

Measured with the committed restatement on the three-plane scene (120 x 200, f 180, base 2.16, T = 3, three fused views; the
fourth view aligned from a guess 0.448 degrees and 0.0838 m off; voxel 0.1, gate 2):
  converged after 5 steps; final error 0.02510 degrees and 0.001361 m; asserted: twice that (MEASURED x 2), because the error is
  structured discretisation noise that moves with the scene's phase against the grid.
  quantised against unquantised final pose: 4.57e-5 degrees and 3.49e-6 m; asserted: twice that."""
import ctypes as C
import math
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

import libviso_amd
from libviso_amd import abi

import align_cases as AC
import align_ref as AR
import tsdf_tables as TT
from estimator_util import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = (0.02510, 0.001361)             # degrees, metres: the final error at voxel 0.1, gate 2
MEASURED_QUANT = (4.57e-5, 3.49e-6)        # quantised against unquantised


@pytest.mark.parametrize("shape", [(3, 130), (1, 1), (37, 333)])
def test_the_two_restatements_agree(shape):
    prm = AC.wide_param(shape)
    m = AC.raycast(AC.FUSED[1], shape, prm)
    e = AC.model(0.1, 3)
    for pose in (AC.FUSED[1], AC.perturbed(AC.FUSED[1])):
        trace = Counter()
        N, c = AR.linearize(e, 0.1, m, prm, pose, gate_voxels=2.0)
        Nl, cl = AR.linearize_loop(e, 0.1, m, prm, pose, gate_voxels=2.0, trace=trace)
        assert N.dtype == np.int64 and N.tobytes() == Nl.tobytes() and c == cl
        assert (N == N.T).all() and c["n_used"] == trace["used"] > 0
        assert sum(trace.values()) == m.size and sum(c[k] for k in AR.COUNTERS[1:]) == c["n_points"]


def test_the_two_restatements_agree_on_every_rule():
    """A random block, a map with invalid and small disparities, a gate of one voxel: every rule but the clip ends some pixel; the
    clip on a view 0.27 m before a wall, the key range a million metres away."""
    e, m = AC.block(), AC.block_map()
    for pose in (None, AC.perturbed(np.eye(4))):
        trace = Counter()
        N, c = AR.linearize(e, 0.2, m, AC.BLOCK_PARAM, pose, min_weight=1)
        Nl, cl = AR.linearize_loop(e, 0.2, m, AC.BLOCK_PARAM, pose, min_weight=1, trace=trace)
        assert N.tobytes() == Nl.tobytes() and c == cl
        assert all(trace[k] > 0 for k in ("invalid", "missing", "gated", "used")), dict(trace)
    shape = (3, 130)
    prm = AC.wide_param(shape)
    m = AC.raycast(AC.CLOSE, shape, prm)
    for pose, rule in ((AC.CLOSE, "clipped"), (AC.view(tx=1e6), "out_of_range")):
        trace = Counter()
        N, c = AR.linearize(AC.model(0.1, 3), 0.1, m, prm, pose, gate_voxels=2.0)
        Nl, cl = AR.linearize_loop(AC.model(0.1, 3), 0.1, m, prm, pose, gate_voxels=2.0, trace=trace)
        assert N.tobytes() == Nl.tobytes() and c == cl and trace[rule] > 0, (rule, dict(trace))


def test_gradient_against_central_differences():
    """psi of step 5 is multilinear in t, so inside one cell its central difference along an axis is the derivative up to rounding."""
    rng = np.random.default_rng(3)
    for _ in range(50):
        m = rng.uniform(-3072, 3072, (2, 2, 2)).tolist()
        t = rng.uniform(0.05, 0.95, 3)
        psi, D = AR.trilinear(m, t)
        h = 0.03
        for ax in range(3):
            lo, hi = t.copy(), t.copy()
            lo[ax] -= h
            hi[ax] += h
            diff = (AR.trilinear(m, hi)[0] - AR.trilinear(m, lo)[0]) / (2 * h)
            assert abs(diff - D[ax]) <= 1e-9 * 3072, (ax, diff, D[ax])
        corner = AR.trilinear(m, (1.0, 0.0, 1.0))[0]
        assert abs(corner - m[1][0][1]) <= 1e-9 and abs(psi) <= 3072   # m[dz][dy][dx] at t = (1, 0, 1), up to rounding


def test_struct_sizes_and_offsets(tmp_path):
    """The structs of the header as a C compiler lays them out against the ctypes and numpy declarations."""
    fields = {"viso_tsdf_align_params": ("min_weight", "gate_voxels", "max_iters", "eps_rot", "eps_trans", "min_pixels"),
              "viso_tsdf_normal": ("n",) + AR.COUNTERS,
              "viso_tsdf_alignment": ("pose", "cov", "cost", "n_used", "iters", "status"),
              "viso_tsdf_align_step": ("pose", "normal")}
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
    P = abi.TsdfAlignParams
    assert got["viso_tsdf_align_params"] == [C.sizeof(P)] + [getattr(P, n).offset for n in fields["viso_tsdf_align_params"]] == [48, 0, 8, 16, 24, 32, 40]
    for s, dt in (("viso_tsdf_normal", abi.TSDF_NORMAL_DTYPE), ("viso_tsdf_alignment", abi.TSDF_ALIGNMENT_DTYPE),
                  ("viso_tsdf_align_step", abi.TSDF_ALIGN_STEP_DTYPE)):
        assert got[s] == [dt.itemsize] + [dt.fields[n][1] for n in fields[s]], s
    assert [got[s][0] for s in ("viso_tsdf_normal", "viso_tsdf_alignment", "viso_tsdf_align_step")] == [272, 440, 400]
    p = libviso_amd.tsdf_align_params()
    assert p.ok() and {k: getattr(p, k) for k in abi.TSDF_ALIGN_DEFAULTS} == AR.DEFAULTS == abi.TSDF_ALIGN_DEFAULTS
    with pytest.raises(TypeError):
        libviso_amd.tsdf_align_params(gate=1.0)


def test_symbols_are_declared_and_exported():
    L = libviso_amd.load()
    assert len(L.viso_tsdf_linearize.argtypes) == 8 and len(L.viso_tsdf_align.argtypes) == 10 and len(L.viso_batch_align_tsdf.argtypes) == 7
    q = abi.TsdfAlignParams()
    L.viso_tsdf_align_params_default(C.byref(q))
    assert {k: getattr(q, k) for k in abi.TSDF_ALIGN_DEFAULTS} == abi.TSDF_ALIGN_DEFAULTS
    assert all(callable(f) for f in (libviso_amd.TsdfMap.linearize, libviso_amd.TsdfMap.align, libviso_amd.Batch.align_tsdf))


def test_argument_errors_with_any_handle():
    """What does not need the map is checked before the handle: every such error answers with VISO_ERR_ARG and "bad argument"
    whatever the handle is, and follows no pointer of it.  With good arguments a handle that is not a live TSDF map is refused."""
    L = libviso_amd.load()
    prm = TT.param()
    d = np.full((2, 3), 300, np.int16)
    out, rec, steps = np.zeros(1, abi.TSDF_NORMAL_DTYPE), np.zeros(1, abi.TSDF_ALIGNMENT_DTYPE), np.zeros(3, abi.TSDF_ALIGN_STEP_DTYPE)
    T = np.eye(4)
    dp, Tp = d.ctypes.data_as(C.POINTER(C.c_int16)), T.ctypes.data_as(C.POINTER(C.c_double))

    def params(**kw):
        p = libviso_amd.tsdf_align_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return C.byref(p)

    def bad_param(**kw):
        p = TT.param()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def linearize(handle, p=None, disp=dp, rows=2, cols=3, param=prm, pose=Tp, o=out.ctypes.data):
        return L.viso_tsdf_linearize(handle, params() if p is None else p, disp, rows, cols, C.byref(param) if param is not None else None, pose, o)

    def align(handle, p=None, disp=dp, rows=2, cols=3, param=prm, pose=Tp, o=rec.ctypes.data, trace=steps.ctypes.data, cap=3):
        return L.viso_tsdf_align(handle, params() if p is None else p, disp, rows, cols, C.byref(param) if param is not None else None, pose, o,
                                 trace, cap)

    Tbad = T.copy()
    Tbad[1, 3] = np.nan
    wrong = [dict(p=C.POINTER(abi.TsdfAlignParams)()), dict(p=params(min_weight=0)), dict(p=params(gate_voxels=0.0)),
             dict(p=params(gate_voxels=-1.0)), dict(p=params(gate_voxels=np.inf)), dict(p=params(gate_voxels=np.nan)), dict(p=params(max_iters=0)),
             dict(p=params(max_iters=51)), dict(p=params(eps_rot=-1e-9)), dict(p=params(eps_rot=np.nan)), dict(p=params(eps_trans=np.inf)),
             dict(p=params(min_pixels=5)), dict(disp=None), dict(param=None), dict(o=None), dict(rows=0), dict(cols=0), dict(rows=-1),
             dict(rows=2048, cols=2049), dict(pose=Tbad.ctypes.data_as(C.POINTER(C.c_double))), dict(param=bad_param(f=0.0)),
             dict(param=bad_param(base=-1.0)), dict(param=bad_param(cu=np.nan)), dict(param=bad_param(cv=np.inf)), dict(param=bad_param(f=np.inf))]
    for handle in (None, C.c_void_p(4096)):
        for name, call in (("viso_tsdf_linearize", linearize), ("viso_tsdf_align", align)):
            for kw in wrong:
                assert call(handle, **kw) == -1, (name, kw)
                msg = L.viso_last_error()
                assert name.encode() in msg and b"bad argument" in msg, (name, kw, msg)
            assert call(handle) == -1 and (name + ": not a live TSDF handle").encode() in L.viso_last_error()
            assert call(handle, pose=None) == -1 and b"not a live" in L.viso_last_error()
        assert align(handle, cap=-1) == -1 and b"bad argument" in L.viso_last_error()
        assert align(handle, trace=None, cap=2) == -1 and b"bad argument" in L.viso_last_error()
        # the resident path: a batch that is not live is refused before the map is looked at
        assert L.viso_batch_align_tsdf(handle, handle, 0, 1, Tp, params(), rec.ctypes.data) == -1
        assert L.viso_batch_align_tsdf(handle, handle, 0, 1, Tp, None, rec.ctypes.data) == -1 and b"bad argument" in L.viso_last_error()
    assert not out.tobytes().strip(b"\0") and not rec.tobytes().strip(b"\0") and not steps.tobytes().strip(b"\0")
    m = object.__new__(libviso_amd.TsdfMap)
    m.L, m.h = L, 4096
    try:
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            m.linearize(d, prm)
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            m.align(d, prm, trace=True)
        with pytest.raises(ValueError):
            m.align(d, prm, pose=np.eye(3))
        with pytest.raises(ValueError):
            m.linearize(d.astype(np.int32), prm)
        with pytest.raises(TypeError):
            m.linearize(d, prm, gate=2.0)
    finally:
        m.h = None


def test_linearize_kernel_has_no_scratch():
    occ, scratch = kernel_resources("tsdf_align.hip", ("tsdf_linearize_kernel",))["tsdf_linearize_kernel"]
    print(f"tsdf_linearize_kernel: occupancy {occ}, scratch {scratch}")
    assert scratch == 0 and occ >= 2


def test_a_single_wall_is_degenerate_and_too_few_pixels_are_refused():
    """A fronto-parallel wall holds the depth and two rotations; the three motions inside it are free: status -2.  Fewer used pixels
    than min_pixels: status -1.  Both return the guess and zeros."""
    c = TT.weights_and_means()
    prm = c[2]
    m = np.full(c[3], int(round(prm.f * prm.base / 2.2 * 16)), np.int16)
    N, cnt = AR.linearize(c[0], 0.2, m, prm, None, min_weight=1)
    assert cnt["n_used"] > 500
    rec, steps = AR.align(c[0], 0.2, m, prm, None, min_weight=1)
    assert rec["status"] == -2 and len(steps) == 1 and rec["iters"] == 0 and rec["n_used"] == 0 and not rec["cov"].any()
    assert (rec["pose"] == np.eye(4)).all()
    prm, e = AC.param(), AC.model(0.1, 3)
    rec, steps = AR.align(e, 0.1, AC.raycast(AC.TRUTH)[:2, :90], prm, AC.GUESS, gate_voxels=2.0)
    assert rec["status"] == -1 and len(steps) == 1 and 0 < steps[0][2]["n_used"] < 200 and (rec["pose"] == AC.GUESS).all()


def test_convergence_on_the_three_plane_scene():
    prm, e, m = AC.param(), AC.model(0.1, 3), AC.raycast(AC.TRUTH)
    guess_err = AR.pose_error(AC.GUESS, AC.TRUTH)
    assert abs(guess_err[0] - 0.45) < 0.01 and abs(guess_err[1] - 0.084) < 0.001
    rec, steps = AR.align(e, 0.1, m, prm, AC.GUESS, gate_voxels=2.0)
    err = AR.pose_error(rec["pose"], AC.TRUTH)
    print(f"status {rec['status']}, {rec['iters']} steps, {rec['n_used']} of {m.size} pixels, cost {rec['cost']:.4f} px, "
          f"error {err[0]:.5f} degrees {err[1]:.6f} m (guess {guess_err[0]:.3f} degrees {guess_err[1]:.4f} m)")
    assert rec["status"] == 1 and rec["iters"] < 10 and len(steps) == rec["iters"] + 1 and rec["n_used"] >= m.size // 2
    assert err[0] <= 2 * MEASURED[0] and err[1] <= 2 * MEASURED[1]
    assert err[0] < guess_err[0] and err[1] < guess_err[1]
    # the largest quantised entry is far below the clip
    assert steps[0][2]["n_clipped"] == 0 and max(int(np.abs(np.diag(N)).max()) for _, N, _ in steps) < 24000 * (1 << 40)
    # the covariance: symmetric and positive definite
    cov = rec["cov"]
    assert np.allclose(cov, cov.T, rtol=1e-9, atol=0) and (np.linalg.eigvalsh((cov + cov.T) / 2) > 0).all()
    # the integers cost nothing: the unquantised rows end at the same pose
    rec_u, _ = AR.align(e, 0.1, m, prm, AC.GUESS, gate_voxels=2.0, quantize=False)
    d = AR.pose_error(rec["pose"], rec_u["pose"])
    print(f"quantised against unquantised: {d[0]:.3e} degrees {d[1]:.3e} m")
    assert rec_u["status"] == 1 and d[0] <= 2 * MEASURED_QUANT[0] and d[1] <= 2 * MEASURED_QUANT[1]
