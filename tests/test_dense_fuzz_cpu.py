"""The generators of tests/dense_fuzz.py without a device: on the restatements alone, the cases that tests/test_gpu_dense_fuzz.py
runs (the same SEEDS and COUNTS, imported from dense_fuzz) reach every launch seam the fuzz is there for, leave the restatements
something to decide (maps with valid and invalid pixels, filters that remove and keep), and are the same cases every time."""
import itertools

import numpy as np
import pytest

import dense_fuzz as F
import speckle_ref as K

INV = F.INVALID


@pytest.fixture(scope="module")
def ran():
    """kind -> [(case, restatement output)] over every seed, computed once."""
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = [(c, F.expected(c)) for seed in F.SEEDS for c in F.CASES[kind](seed, F.COUNTS[kind])]
        return cache[kind]
    return get


def _cases(kind):
    return [c for seed in F.SEEDS for c in F.CASES[kind](seed, F.COUNTS[kind])]


def test_block_matching_reaches_every_thread_run_and_the_lds_line():
    cs = _cases("bm")
    computed = [c for c in cs if min(c["L"].shape) >= c["params"]["block"]]   # the kernel leaves at once below that
    runs = {F.bm_run(c["L"].shape[1]) for c in computed}
    ks = {F.bm_k(c["params"]["block"]) for c in computed}
    print("runs", sorted(runs), "K", sorted(ks))
    assert runs == set(range(1, 9)) and ks == set(range(2, 7))
    assert {c["params"]["block"] for c in computed} == set(F.BLOCKS) and {c["params"]["num_disp"] for c in cs} == set(F.NUM_DISPS)
    widths = {c["L"].shape[1] for c in computed}
    assert set(F.WIDTH_SEAMS) <= widths and len(F.WIDTH_SEAMS) == 23
    above = [c for c in computed if F.bm_above_lds_line(c["params"]["block"], c["L"].shape[1])]
    print("above the 64 KiB line:", len(above), "with K", sorted({F.bm_k(c["params"]["block"]) for c in above}))
    assert len(above) >= 5
    assert any(c["L"].shape[1] == 1241 and c["params"]["block"] == 21 for c in above)
    assert {F.bm_k(c["params"]["block"]) for c in above} == {4, 5, 6}         # K <= 3 never crosses it below 2049 columns
    # the first width past the line of a K, and the widest image
    assert any(F.bm_lds_bytes(c["params"]["block"], c["L"].shape[1] - 1) <= 65536 for c in above)
    # dlim = cols - 1 - 2r below D - 1, and the window's own seams
    assert sum(c["L"].shape[1] - c["params"]["block"] < c["params"]["num_disp"] - 1 for c in computed) >= 10
    assert any(c["L"].shape[1] == c["params"]["block"] for c in cs) and any(c["L"].shape[1] == c["params"]["block"] - 1 for c in cs)
    assert any(c["L"].shape[0] == c["params"]["block"] for c in cs) and any(c["L"].shape[0] == c["params"]["block"] - 1 for c in cs)
    # the parameters' ends
    for key, ends in (("prefilter_cap", (1, 2, 62, 63)), ("uniqueness", (0, 1, 99, 100)), ("texture_threshold", (0, 1, F.TEX_HUGE))):
        assert set(ends) <= {c["params"][key] for c in cs}, key
    assert {-1, 0, 1} <= {c["params"]["lr_max_diff"] for c in cs}
    assert sum(c["params"]["lr_max_diff"] == c["params"]["num_disp"] for c in cs) >= 10
    assert {c["image"] for c in cs} == set(F.IMAGE_CLASSES)


def test_sgm_reaches_every_lane_count_and_the_tall_wrap():
    cs = _cases("sgm")
    assert {(F.sgm_k(c["params"]["num_disp"]), c["params"]["paths"]) for c in cs} == set(itertools.product((1, 2, 3, 4), (4, 8)))
    assert {c["params"]["num_disp"] for c in cs} == set(F.NUM_DISPS)
    tall = sum(c["L"].shape[0] > c["L"].shape[1] > 1 for c in cs)
    tall8 = sum(c["L"].shape[0] > c["L"].shape[1] > 1 and c["params"]["paths"] == 8 for c in cs)   # the diagonals are the last four
    short = sum(c["params"]["num_disp"] > c["L"].shape[1] for c in cs)
    print("rows > cols > 1:", tall, "of them with 8 paths:", tall8, "num_disp > cols:", short)
    assert tall >= 10 and tall8 >= 10 and short >= 10
    assert set(F.WIDTH_SEAMS) <= {c["L"].shape[1] for c in cs}
    assert any(c["L"].shape[1] == 1 for c in cs) and any(c["L"].shape[0] == 1 for c in cs)
    pp = {(c["params"]["p1"], c["params"]["p2"]) for c in cs}
    assert (1, 1) in pp and (191, 191) in pp and (192, 192) in pp and any(a < b == 191 for a, b in pp) and any(a < b == 192 for a, b in pp)
    assert all(1 <= a <= b <= 192 for a, b in pp)
    assert {0, 1, 99, 100} <= {c["params"]["uniqueness"] for c in cs} and {-1, 0, 1} <= {c["params"]["lr_max_diff"] for c in cs}
    assert sum(c["params"]["lr_max_diff"] == c["params"]["num_disp"] for c in cs) >= 10
    assert {c["image"] for c in cs} == set(F.IMAGE_CLASSES)


def test_rectify_reaches_every_frame_chunk_and_store_path():
    cs = _cases("rectify")
    nfs = {c["raw"].shape[0] for c in cs}
    assert nfs == set(F.FRAME_COUNTS)
    for lo, hi in ((1, 31), (32, 32), (33, 63), (64, 64), (65, 96)):   # below, at and above one chunk and two
        assert any(lo <= n <= hi for n in nfs), (lo, hi)
    pers = [c["out_shape"][0] * c["out_shape"][1] for c in cs]
    assert {p % 4 for p in pers} == {0, 1, 2, 3}
    # each store path past the first frame chunk, and partial last tiles on both
    for res in range(4):
        assert any(p % 4 == res and c["raw"].shape[0] > F.RECT_FPB for p, c in zip(pers, cs)), res
    for k in (1, 2, 3):
        near = {p - k * F.RECT_TILE for p in pers if abs(p - k * F.RECT_TILE) <= 3}
        assert {-1, 0, 1} <= near, (k, near)
    assert {0, 255} <= {c["border"] for c in cs}
    assert all(c["mapx"].shape == tuple(c["out_shape"]) == c["mapy"].shape for c in cs)


def test_speckle_thresholds_sit_on_component_sizes(ran):
    done = ran("speckle")
    at = 0
    for c, _ in done:
        sizes = K.component_sizes(c["map"], c["params"]["max_diff"])
        present = set(np.unique(sizes[sizes > 0]).tolist())
        s = c["params"]["max_size"]
        at += s in present or s + 1 in present
    both = sum(bool((out != c["map"]).any() and (out != INV).any()) for c, out in done)
    print("max_size at a component's size or one below: %d of %d; removes and keeps: %d" % (at, len(done), both))
    assert 4 * at >= len(done)
    assert 2 * both >= len(done)
    cs = [c for c, _ in done]
    assert {c["params"]["max_diff"] for c in cs} == set(F.MAX_DIFFS)
    assert {0, 1} <= {c["params"]["max_size"] for c in cs} and any(c["params"]["max_size"] == c["map"].size for c in cs)
    rows, cols = {c["map"].shape[0] for c in cs}, {c["map"].shape[1] for c in cs}
    assert {F.SPK_TH * k + e for k in (1, 2, 3) for e in (-1, 0, 1)} <= rows and 1 in rows
    assert {F.SPK_TW * k + e for k in (1, 2, 3, 4) for e in (-1, 0, 1)} <= cols and 1 in cols
    assert any(c["map"].max() == 32767 for c in cs) and any(c["map"].min() == -32768 for c in cs)
    assert {"serpentine", "vertical serpentine", "comb"} <= {c["image"] for c in cs}


@pytest.mark.parametrize("kind", ["bm", "sgm"])
def test_maps_have_valid_and_invalid_pixels(ran, kind):
    done = ran(kind)
    mixed = sum(bool((out != INV).any() and (out == INV).any()) for _, out in done)
    empty = sum(not (out != INV).any() for _, out in done)
    print("%s: %d cases, %d with valid and invalid pixels, %d all invalid" % (kind, len(done), mixed, empty))
    assert 2 * mixed >= len(done)
    assert 3 * empty <= len(done)
    for seed in F.SEEDS:   # and no seed on its own is degenerate
        part = [out for c, out in done if c["seed"] == seed]
        assert 2 * sum(bool((out != INV).any() and (out == INV).any()) for out in part) >= len(part), seed


def test_points_cases_use_every_branch():
    cs = _cases("points")
    assert any(c["pose"] is None for c in cs) and any(c["pose"] is not None and c["pose"].shape == (4, 4) for c in cs)
    assert any(c["pose"] is not None and c["pose"].shape == (3, 4) for c in cs)
    assert {1, 16, 160} <= {c["min_disp16"] for c in cs}
    for c in cs:
        m = c["map"]
        assert (m == INV).any() or m.size < 8
    assert sum(bool(((c["map"] != INV) & (c["map"] < c["min_disp16"])).any()) for c in cs) >= len(cs) // 2
    assert {-1, 0, 1} <= {c["map"].size % 256 if c["map"].size % 256 < 2 else c["map"].size % 256 - 256 for c in cs}


@pytest.mark.parametrize("kind", F.KERNELS)
def test_generators_are_deterministic(kind):
    n = min(F.COUNTS[kind], 40)
    for seed in F.SEEDS[:2]:
        a = [F.case_digest(c) for c in F.CASES[kind](seed, n)]
        b = [F.case_digest(c) for c in F.CASES[kind](seed, n)]
        assert a == b and len(set(a)) == n
        # a case does not depend on how many are asked for, so a reported (seed, index) is enough to run it again
        assert [F.case_digest(c) for c in F.CASES[kind](seed, 7)] == a[:7]
    c = next(iter(F.CASES[kind](0, 1)))
    text = F.describe(c)
    assert "seed 0 index 0" in text and kind in text
    other = next(iter(F.CASES[kind](1, 1)))
    assert F.case_digest(other) != F.case_digest(c)


def test_the_module_needs_no_library():
    """Importing dense_fuzz and drawing cases loads no shared library: the generators are numpy."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = ("import sys; sys.path.insert(0, %r); import dense_fuzz as F\n"
            "assert 'libviso_amd' not in sys.modules\n"
            "for k in F.KERNELS: list(F.CASES[k](0, 3))\n"
            "import libviso_amd; assert libviso_amd._lib is None and 'torch' not in sys.modules") % here
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
