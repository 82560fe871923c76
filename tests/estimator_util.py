"""Helpers shared by the tests of the opt-in fp64 motion estimators (covariance.hip, refine.hip, window.hip): a batch over a
synthetic sequence with the estimators set, the restatements' rounding-level decisions, the per-case bounds of a device record
against a restatement's (from its `slack`), and the compiler's resource usage of a kernel."""
import os
import re
import subprocess
import tempfile

import numpy as np

import libviso_amd
from libviso_amd.abi import MatchParams


def seq_batch(ctx, seq, seed=3, first=0, frames=None, cov=(0,), refine=(0,), window=(0,)):
    """A Batch over seq's frames (a slice, or all), run once with the estimators set as given: cov and refine the arguments of
    set_covariance / set_refine (mode, sigma), window those of set_window_refine (K, mode, sigma)."""
    sl = slice(None) if frames is None else frames
    kp, desc, n = (np.ascontiguousarray(seq[k][sl]) for k in ("kp", "desc", "n"))
    nf, cap = kp.shape[0], kp.shape[2]
    b = libviso_amd.Batch(ctx, nf, cap)
    b.upload(kp, desc, n)
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=seed, first_frame=first)
    b.set_covariance(*cov)
    b.set_refine(*refine)
    b.set_window_refine(*window)
    b.run()
    return b


def ambiguous(want):
    """True when one of the restatement's decisions compared costs that differ by less than 1e-11 relative -- the accept test
    (C_new < C) and the stop test (C - C_new <= 1e-12 C) near their thresholds: there the device, whose sums run in another order,
    may take the other branch (one accepted step more or less, of a size at rounding level).  Every run that converges ends on such
    a decision, so this guards `iters` alone (equal, or within 1); what the state may differ by comes from `slack` (bound)."""
    return any(abs(d) < 1e-11 for d in want["trace"])


def check_iters(got_iters, want, what):
    assert abs(int(got_iters) - want["iters"]) <= (1 if ambiguous(want) else 0), (what, int(got_iters), want["iters"])


GAPS = {}                        # quantity: (largest device-to-restatement gap seen in this process, its bound, the case)


def note_gap(name, gap, limit, what):
    if gap >= GAPS.get(name, (-1.0,))[0]:
        GAPS[name] = (gap, limit, what)


# quantity: (strict, loose).  strict holds for a device that takes the restatement's decisions; loose was the bound of a run with a
# rounding-level decision before the bounds became per case, and none may exceed it.
TR_WHITE = (1e-5, 1e-4)          # tr, in units of its own standard deviation
TR_ABS = (1e-8, 1e-6)            # |tr - tr_ref|, n >= 40 points
TR_ABS_SMALL = (1e-7, 1e-6)      # the same, n < 40
WIN_ABS = (1e-7, 1e-6)           # the window's tr_win
PTS_REL = (1e-7, 1e-6)           # a point's coordinates, relative to the largest |coordinate| of all
PTS_WHITE = (1e-5, 1e-4)         # a point, in units of its own standard deviation (whitened by its undamped Hpp)
SLACK_STEPS = 4                  # the device may take one or two rounding-level accepted steps more or fewer; rejected ones move nothing


def raw_bound(limits, slack):
    """strict + 4 x slack: the bound of one quantity of one case, from the restatement's own last steps."""
    return limits[0] + SLACK_STEPS * slack


def bound(limits, slack):
    """raw_bound, never above the loose value.  The cap binds only where a run ends away from convergence (the LM_MAX_ACCEPT and
    LM_MAX_REJECT exits), whose last steps are large: there the device follows the restatement's decisions or fails."""
    return min(raw_bound(limits, slack), limits[1])


def tr_abs_limits(n):
    return TR_ABS if n >= 40 else TR_ABS_SMALL


def gap_tolerance(want):
    """What sqrt(gap) may differ by where the restatement ends away from convergence (gap > 1e-6).  sqrt(gap) is the whitened length
    of the Gauss-Newton step of tr that is left at the final state: a smooth function of the state whose derivative is -1 along tr
    for a linear model.  Two final states within the bounds of tr and of the points, both whitened, so differ by their sum in
    sqrt(gap); the factor 4 leaves room for the curvature away from the optimum, and 1e-6 relative for the covariance's 1e-7."""
    sl = want["slack"]
    return 4.0 * (bound(TR_WHITE, sl["tr_white"]) + bound(PTS_WHITE, sl["pts_white"])) + 1e-6 * np.sqrt(want["gap"])


def check_gap(got_gap, want, what, far=False):
    """gap is below 1e-6 on both sides.  far: a case that may end away from convergence (an LM_MAX_ACCEPT or LM_MAX_REJECT exit);
    where it does, the device's gap equals the restatement's within gap_tolerance."""
    if not far or want["gap"] <= 1e-6:
        assert got_gap <= 1e-6 and want["gap"] <= 1e-6, (what, got_gap, want["gap"])
    else:
        assert abs(np.sqrt(got_gap) - np.sqrt(want["gap"])) <= gap_tolerance(want), (what, got_gap, want["gap"])


def check_points(pts, want, what):
    """Refined points (3, n) of the device against the restatement's (3, n), status 1: relative to the largest coordinate, and every
    point whitened by its own undamped Hpp at the restatement's final state.  Returns the two figures."""
    ref, sl = want["points"], want["slack"]
    assert pts.shape == ref.shape, (what, pts.shape, ref.shape)
    assert np.all(np.isfinite(pts)), what
    d = pts - ref
    rel = float(np.abs(d).max() / np.abs(ref).max())
    white = float(np.sqrt(np.einsum("an,nac,cn->n", d, want["Hpp"], d).max()))
    note_gap("refine points relative", rel, bound(PTS_REL, sl["pts_rel"]), what)
    note_gap("refine points whitened", white, bound(PTS_WHITE, sl["pts_white"]), what)
    assert rel <= bound(PTS_REL, sl["pts_rel"]), (what, rel, sl["pts_rel"])
    assert white <= bound(PTS_WHITE, sl["pts_white"]), (what, white, sl["pts_white"])
    return rel, white


def kernel_resources(src_name, kernels):
    """Compile libviso_amd/csrc/<src_name> for gfx950 and read -Rpass-analysis=kernel-resource-usage: {kernel: (occupancy in
    waves per SIMD, scratch bytes per lane)}."""
    src = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "csrc", src_name)
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                            "-fno-fast-math", "-c", src, "-o", os.path.join(tmp, "k.o"), "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for name in kernels:
        i = r.stderr.index(name)
        block = r.stderr[i:i + 4000]
        out[name] = (int(re.search(r"Occupancy \[waves/SIMD\]: (\d+)", block).group(1)),
                     int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", block).group(1)))
    return out
