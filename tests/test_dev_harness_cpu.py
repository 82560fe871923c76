"""The test-only harness of the device helper headers, without a GPU: it compiles for gfx950 with the library's flags and exports
every wrapper; it covers every DPP control, row mask, swizzle pattern and block_sum instantiation the library uses; the numpy lane
models of tests/wave_ref.py agree with source-lane tables written out by hand and with numpy's own reductions (what makes them a
reference for tests/test_gpu_dev_helpers.py and not a second copy); and no comparator of bitonic_sort_lds reaches past its keys."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

import dev_harness as H
import wave_ref as W

N = -1   # a lane without a source
# the lane every lane reads, per DPP control listed at the top of wave.h
SOURCES = {
    0xB1: [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 13, 12, 15, 14, 17, 16, 19, 18, 21, 20, 23, 22, 25, 24, 27, 26, 29, 28, 31, 30,
           33, 32, 35, 34, 37, 36, 39, 38, 41, 40, 43, 42, 45, 44, 47, 46, 49, 48, 51, 50, 53, 52, 55, 54, 57, 56, 59, 58, 61, 60, 63, 62],
    0x4E: [2, 3, 0, 1, 6, 7, 4, 5, 10, 11, 8, 9, 14, 15, 12, 13, 18, 19, 16, 17, 22, 23, 20, 21, 26, 27, 24, 25, 30, 31, 28, 29,
           34, 35, 32, 33, 38, 39, 36, 37, 42, 43, 40, 41, 46, 47, 44, 45, 50, 51, 48, 49, 54, 55, 52, 53, 58, 59, 56, 57, 62, 63, 60, 61],
    0x00: [0, 0, 0, 0, 4, 4, 4, 4, 8, 8, 8, 8, 12, 12, 12, 12, 16, 16, 16, 16, 20, 20, 20, 20, 24, 24, 24, 24, 28, 28, 28, 28,
           32, 32, 32, 32, 36, 36, 36, 36, 40, 40, 40, 40, 44, 44, 44, 44, 48, 48, 48, 48, 52, 52, 52, 52, 56, 56, 56, 56, 60, 60, 60, 60],
    0x55: [1, 1, 1, 1, 5, 5, 5, 5, 9, 9, 9, 9, 13, 13, 13, 13, 17, 17, 17, 17, 21, 21, 21, 21, 25, 25, 25, 25, 29, 29, 29, 29,
           33, 33, 33, 33, 37, 37, 37, 37, 41, 41, 41, 41, 45, 45, 45, 45, 49, 49, 49, 49, 53, 53, 53, 53, 57, 57, 57, 57, 61, 61, 61, 61],
    0xAA: [2, 2, 2, 2, 6, 6, 6, 6, 10, 10, 10, 10, 14, 14, 14, 14, 18, 18, 18, 18, 22, 22, 22, 22, 26, 26, 26, 26, 30, 30, 30, 30,
           34, 34, 34, 34, 38, 38, 38, 38, 42, 42, 42, 42, 46, 46, 46, 46, 50, 50, 50, 50, 54, 54, 54, 54, 58, 58, 58, 58, 62, 62, 62, 62],
    0xFF: [3, 3, 3, 3, 7, 7, 7, 7, 11, 11, 11, 11, 15, 15, 15, 15, 19, 19, 19, 19, 23, 23, 23, 23, 27, 27, 27, 27, 31, 31, 31, 31,
           35, 35, 35, 35, 39, 39, 39, 39, 43, 43, 43, 43, 47, 47, 47, 47, 51, 51, 51, 51, 55, 55, 55, 55, 59, 59, 59, 59, 63, 63, 63, 63],
    0x101: [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, N, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, N,
            33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, N, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, N],
    0x111: [N, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, N, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30,
            N, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, N, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62],
    0x112: [N, N, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, N, N, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
            N, N, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, N, N, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61],
    0x113: [N, N, N, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, N, N, N, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28,
            N, N, N, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, N, N, N, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60],
    0x114: [N, N, N, N, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, N, N, N, N, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27,
            N, N, N, N, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, N, N, N, N, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59],
    0x115: [N, N, N, N, N, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, N, N, N, N, N, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26,
            N, N, N, N, N, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, N, N, N, N, N, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58],
    0x116: [N, N, N, N, N, N, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, N, N, N, N, N, N, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25,
            N, N, N, N, N, N, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, N, N, N, N, N, N, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57],
    0x117: [N, N, N, N, N, N, N, 0, 1, 2, 3, 4, 5, 6, 7, 8, N, N, N, N, N, N, N, 16, 17, 18, 19, 20, 21, 22, 23, 24,
            N, N, N, N, N, N, N, 32, 33, 34, 35, 36, 37, 38, 39, 40, N, N, N, N, N, N, N, 48, 49, 50, 51, 52, 53, 54, 55, 56],
    0x118: [N, N, N, N, N, N, N, N, 0, 1, 2, 3, 4, 5, 6, 7, N, N, N, N, N, N, N, N, 16, 17, 18, 19, 20, 21, 22, 23,
            N, N, N, N, N, N, N, N, 32, 33, 34, 35, 36, 37, 38, 39, N, N, N, N, N, N, N, N, 48, 49, 50, 51, 52, 53, 54, 55],
    0x128: [8, 9, 10, 11, 12, 13, 14, 15, 0, 1, 2, 3, 4, 5, 6, 7, 24, 25, 26, 27, 28, 29, 30, 31, 16, 17, 18, 19, 20, 21, 22, 23,
            40, 41, 42, 43, 44, 45, 46, 47, 32, 33, 34, 35, 36, 37, 38, 39, 56, 57, 58, 59, 60, 61, 62, 63, 48, 49, 50, 51, 52, 53, 54, 55],
    0x130: [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32,
            33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, N],
    0x138: [N, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30,
            31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62],
    0x140: [15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0, 31, 30, 29, 28, 27, 26, 25, 24, 23, 22, 21, 20, 19, 18, 17, 16,
            47, 46, 45, 44, 43, 42, 41, 40, 39, 38, 37, 36, 35, 34, 33, 32, 63, 62, 61, 60, 59, 58, 57, 56, 55, 54, 53, 52, 51, 50, 49, 48],
    0x141: [7, 6, 5, 4, 3, 2, 1, 0, 15, 14, 13, 12, 11, 10, 9, 8, 23, 22, 21, 20, 19, 18, 17, 16, 31, 30, 29, 28, 27, 26, 25, 24,
            39, 38, 37, 36, 35, 34, 33, 32, 47, 46, 45, 44, 43, 42, 41, 40, 55, 54, 53, 52, 51, 50, 49, 48, 63, 62, 61, 60, 59, 58, 57, 56],
    0x142: [N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15,
            31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47, 47],
    0x143: [N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N, N,
            31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31, 31],
}


def _csrc_text():
    files = sorted(glob.glob(os.path.join(H.libviso_amd.CSRC, "*.hip")) + glob.glob(os.path.join(H.libviso_amd.CSRC, "*.h")))
    return "\n".join(open(f).read() for f in files)


def test_the_harness_compiles_for_gfx950_and_exports_every_wrapper():
    cmd = H.compile_command("x.so")
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd and "-O3" in cmd and "-shared" in cmd
    lib = ctypes.CDLL(H.build())
    missing = [n for n in H.WRAPPERS if not hasattr(lib, "dh_" + n)]
    assert not missing, missing
    # the GPU tests reach the library through call() (which admits ELEMENTWISE only) and the functions of dev_harness.py
    used = set(re.findall(r"\.dh_(\w+)\(", open(os.path.join(H.HERE, "dev_harness.py")).read()))
    assert used and used <= set(H.OTHERS), used - set(H.OTHERS)
    assert len(set(H.WRAPPERS)) == len(H.WRAPPERS)


def test_the_harness_covers_every_control_and_instantiation_of_the_library():
    text = _csrc_text()
    for c in set(re.findall(r"\bwave_dpp<0x(\w+)>", text)):
        assert "wave_dpp_0x" + c in H.ELEMENTWISE, c
    for c in set(re.findall(r"\bwave_dpp_bc<0x(\w+)>", text)):
        assert "wave_dpp_bc_0x" + c in H.ELEMENTWISE, c
    pairs = set(re.findall(r"\bviso_dpp<0x(\w+), 0x(\w+)>", text))
    steps = re.search(r"#define VISO_WAVE_STEPS\(OP\) (.*)", text).group(1)
    step_pairs = re.findall(r"OP\(0x(\w+), 0x(\w+)\)", steps)
    assert [(int(c, 16), int(m, 16)) for c, m in step_pairs] == list(W.WAVE_STEPS)
    for c, m in pairs | set(step_pairs):
        assert "viso_dpp_0x%s_0x%s" % (c, m) in H.ELEMENTWISE, (c, m)
    for c, m in step_pairs:   # wave_sum_to_lane63 moves doubles by the same steps
        assert "dpp_f64_0x%s_0x%s" % (c, m) in H.ELEMENTWISE, (c, m)
    for c in set(re.findall(r"\bwave_swizzle<0x(\w+)>", text)):
        assert "wave_swizzle_0x" + c in H.ELEMENTWISE, c
    defs = dict(re.findall(r"#define (\w+) (\d+)\b", text))
    assert defs["RF_THREADS"] == defs["COV_THREADS"] == "256"       # WAVES = 4 of both estimators' block_sum
    for ns in set(re.findall(r"\bblock_sum<(\w+), \w+_WAVES>", text)):
        assert "block_sum_%s_4" % defs.get(ns, ns) in H.ELEMENTWISE, ns
    assert defs["VISO_NB"] == "256" and defs["ST_NBY"] == defs["MU_NBY"] == "64"   # the two NB of the harness's bucket kernel
    assert set(re.findall(r"\bbitonic_sort_lds<(\w+)>", text)) == {"VISO_SORT_THREADS"} and defs["VISO_SORT_THREADS"] == "512"
    # every control the header lists is in the table below, and every control in use is listed
    used = {int(c, 16) for c in re.findall(r"\b(?:wave_dpp|wave_dpp_bc|viso_dpp)<0x(\w+)", text)} | {c for c, _ in W.WAVE_STEPS}
    assert used <= set(SOURCES), [hex(c) for c in used - set(SOURCES)]


@pytest.mark.parametrize("ctrl", sorted(SOURCES))
def test_dpp_model_reads_the_lane_written_out_here(ctrl):
    assert W.dpp_source(ctrl).tolist() == SOURCES[ctrl]
    v = (np.arange(64, dtype=np.uint32) + 1) * np.uint32(0x01000193)
    want = np.array([v[s] if s >= 0 else 0xDEAD for s in SOURCES[ctrl]], np.uint32)
    assert np.array_equal(W.dpp(v, ctrl, 0xF, 0xDEAD), want)
    want0 = np.where(np.array(SOURCES[ctrl]) >= 0, want, 0).astype(np.uint32)
    assert np.array_equal(W.dpp(v, ctrl, 0xF, 0xDEAD, bound_ctrl=True), want0)
    for mask in (0xA, 0xC, 0x1):   # the rows outside the mask keep `old`, with and without bound_ctrl
        inside = ((mask >> (np.arange(64) >> 4)) & 1) == 1
        assert np.array_equal(W.dpp(v, ctrl, mask, 0xDEAD), np.where(inside, want, 0xDEAD))
        assert np.array_equal(W.dpp(v, ctrl, mask, 0xDEAD, bound_ctrl=True), np.where(inside, want0, 0xDEAD))


def test_swizzle_model():
    v = np.arange(64) * 3 + 1
    assert np.array_equal(W.swizzle(v, 0x101F), v[np.arange(64) ^ 4])
    assert np.array_equal(W.swizzle(v, 0x401F), v[np.arange(64) ^ 16])
    for i in range(8):
        assert np.array_equal(W.swizzle(v, (i << 5) | 0x18), v[(np.arange(64) & ~7) | i])


def _waves(rng):
    yield rng.integers(0, 2 ** 32, 64, dtype=np.uint64).astype(np.uint32)
    yield rng.integers(0, 5, 64).astype(np.uint32)
    yield np.full(64, 0xFFFFFFFF, np.uint32)
    yield np.zeros(64, np.uint32)
    for lane in (0, 15, 16, 31, 32, 47, 48, 63):
        v = rng.integers(1000, 2000, 64).astype(np.uint32)
        v[lane] = 7
        yield v
        v = v.copy()
        v[lane] = 0xFFFFFF00
        yield v


def test_reduction_models_agree_with_numpy():
    rng = np.random.default_rng(1)
    for v in _waves(rng):
        assert W.wave_min63(v)[63] == v.min() and W.wave_max63(v)[63] == v.max() and W.wave_max_keep(v)[63] == v.max()
        assert np.array_equal(W.wave_scan(v), np.cumsum(v, dtype=np.uint32))
        assert np.array_equal(W.row_min(v), np.repeat(v.reshape(4, 16).min(axis=1), 16))
        assert np.array_equal(W.wave_min_all(v), np.full(64, v.min(), np.uint32))
        assert np.array_equal(W.group_sum(v, 4), np.repeat(v.reshape(16, 4).sum(axis=1, dtype=np.uint32), 4))
        assert np.array_equal(W.group_sum(v, 8), np.repeat(v.reshape(8, 8).sum(axis=1, dtype=np.uint32), 8))
        k = (v.astype(np.uint64) << np.uint64(32)) | np.uint64(5)
        k[::3] |= rng.integers(0, 2 ** 32, len(k[::3]), dtype=np.uint64)
        assert W.wave_max63(k)[63] == k.max() and np.array_equal(W.wave_max_u64(k), np.full(64, k.max(), np.uint64))
        assert W.wave_scan(k)[63] == np.sum(k, dtype=np.uint64)
        f = (v % 4096).astype(np.float32) - 2048            # small integers: every order of additions is exact
        assert W.wave_scan(f)[63] == f.sum(dtype=np.float64) and W.wave_scan(f.astype(np.float64))[63] == f.sum(dtype=np.float64)
        assert np.array_equal(W.wave_fext(f, False), np.full(64, f.min(), np.float32))
        assert np.array_equal(W.wave_fext(f, True), np.full(64, f.max(), np.float32))
        acc = rng.integers(-1000, 1000, (256, 3)).astype(np.float64)
        assert np.array_equal(W.block_sum(acc, 4), acc.sum(axis=0))
    f = rng.normal(0, 1, 64).astype(np.float32)
    f[[3, 40]] = np.nan
    assert W.wave_fext(f, False)[0] == np.nanmin(f) and W.wave_fext(f, True)[17] == np.nanmax(f)
    assert np.isnan(W.wave_fext(np.full(64, np.nan, np.float32), True)).all()
    # the float sums are the six steps' order, not numpy's: a cancellation that only this order loses
    g = np.zeros(64, np.float32)
    g[0], g[1], g[2] = 1e8, 1.0, -1e8
    assert W.wave_scan(g)[63] == 0.0 and float(np.sum(g.astype(np.float64))) == 1.0


def test_small_models():
    assert W.pack_block_sums(np.r_[np.full(16, 3000), np.full(16, -3000), np.full(16, 1), np.zeros(16)].astype(np.int64)) == (0x0000FFFF, 0x80008010)
    assert W.row8([-2000, -128, 0, 127, 128, 5000], 0).tolist() == [0, 0, 128, 255, 255, 255]
    assert W.row8([-2000, -1024, -1, 0, 1016, 1023, 1024], 3).tolist() == [0, 0, 127, 128, 255, 255, 255]
    assert W.splitmix64(0) == (0xE220A8397B1DCDAF, 0x9E3779B97F4A7C15)       # the published first output for seed 0
    assert W.map_hash(0x9E3779B97F4A7C15) == 0x7B1DCDAF


@pytest.mark.parametrize("threads", [256, 512])
def test_no_bitonic_comparator_reaches_past_its_keys(threads):
    """bitonic_sort_lds<THREADS>(keys, npad) may touch keys[0 .. npad) only: its loops restated (wave_ref.bitonic_stages), with the
    comparators per wave and stage read from match_dev.h.  Every stage runs npad / 2 comparators that touch every key once, and the
    network sorts.  (With cw = 64 at npad = 64 wave 0 ran 64 comparators where the network has 32: indices up to 127.)"""
    cw_of = W.bitonic_cw(open(os.path.join(H.CSRC, "match_dev.h")).read())
    rng = np.random.default_rng(threads)
    npad = 64
    while npad <= 16384:     # VISO_SORT_MAX: the largest the sort kernel passes
        for i, l, up in W.bitonic_stages(threads, npad, cw_of):
            assert max(i.max(), l.max()) < npad, (npad, int(max(i.max(), l.max())))
            assert np.array_equal(np.sort(np.r_[i, l]), np.arange(npad)), npad
        if npad <= 2048:
            keys = rng.integers(0, 50, npad).astype(np.uint64)
            assert np.array_equal(W.bitonic_sort_model(keys, threads, cw_of), np.sort(keys)), npad
        npad <<= 1
