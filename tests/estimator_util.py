"""Helpers shared by the tests of the opt-in fp64 motion estimators (covariance.hip, refine.hip, window.hip): a batch over a
synthetic sequence with the estimators set, the restatements' rounding-level decisions, and the compiler's resource usage of a
kernel."""
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
    may take the other branch (one accepted step more or less, of a size at rounding level)."""
    return any(abs(d) < 1e-11 for d in want["trace"])


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
