"""CPU checks of the opt-in sub-pixel stereo refinement's definition (include/viso_hip.h, viso_batch_set_subpixel) through
its numpy restatement (tests/subpixel_ref.py), and of what it buys on a scene built with fractional disparities.  The
thresholds of the last two tests were set from CPU measurements of these seeded scenes, with margin (DESIGN.md
"Sub-pixel stereo refinement")."""
import numpy as np
import pytest

from libviso_amd import synth

import subpixel_ref as S


def test_parabola_offset_hand_cases():
    off = S.parabola_offset
    assert off(7, 7, 7) == 0.0                    # flat cost
    assert off(9, 4, 9) == 0.0                    # symmetric about the centre
    assert off(3, 5, 9) == 0.0                    # S0 not the minimum
    assert off(9, 5, 3) == 0.0
    assert off(10, 4, 6) == 0.25                  # (10 - 6) / (2 * (10 + 6 - 8))
    assert off(6, 4, 10) == -0.25
    assert off(5, 5, 9) == 0.5 * (5 - 9) / (5 + 9 - 10)   # S0 == S-: still a minimum, |off| = 1/2 at most
    assert off(5, 5, 9) == -0.5
    a = np.array([[0, 0, 0], [1, 0, 0], [100, 1, 3]])
    o = off(a[:, 0], a[:, 1], a[:, 2])
    assert o[0] == 0.0 and o[1] == 0.5 and o[2] == 97.0 / (2.0 * 101.0)
    rng = np.random.default_rng(0)
    s = rng.integers(0, 5000, (10000, 3))
    assert np.abs(off(s[:, 0], s[:, 1], s[:, 2])).max() <= 0.5


def _sobel_windows(img, pts):
    """Independent restatement of the extractor: Sobel-x with reflect-101 on the whole image, zero rule per pixel."""
    rows, cols = img.shape
    p = np.pad(img.astype(np.int64), 1, mode="reflect")
    sob = (p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
    out = np.zeros((len(pts), 121), np.int64)
    for k, (x, y) in enumerate(pts):
        c = 0
        for i in range(-5, 6):
            for j in range(-5, 6):
                yy, xx = y + i, x + j
                out[k, c] = sob[yy, xx] if (0 < yy < rows and 0 < xx < cols) else 0
                c += 1
    return out


def test_costs_and_windows_at_the_borders(oracle):
    rows, cols = 40, 52
    imgL = synth.make_images(3, rows, cols)
    imgR = synth.make_images(4, rows, cols)
    edge = [0, 1, 2, cols - 2, cols - 1]
    edgey = [0, 1, rows - 2, rows - 1]
    kp1 = np.array([[x, y] for x in edge for y in edgey] + [[20, 20], [25.5, 10.5], [26.5, 11.4]], np.float32)
    kp2 = kp1[::-1].copy()
    n = len(kp1)
    match = np.stack([np.arange(n), np.arange(n), np.zeros(n)], 1).astype(np.int32)
    Sx, Sy = S.costs(oracle, imgL, imgR, kp1, kp2, match)
    p = np.rint(kp1).astype(int); q = np.rint(kp2).astype(int)
    assert tuple(p[-2]) == (26, 10) and tuple(p[-1]) == (26, 11)   # half to even, like cvRound
    wl = _sobel_windows(imgL, p)
    for c, d in enumerate((-1, 0, 1)):
        wx = _sobel_windows(imgR, q + [d, 0])
        wy = _sobel_windows(imgR, q + [0, d])
        assert np.array_equal(Sx[:, c], np.abs(wl - wx).sum(1))
        assert np.array_equal(Sy[:, c], np.abs(wl - wy).sum(1))
    assert np.array_equal(Sx[:, 1], Sy[:, 1])
    d = oracle.extract_descriptors(imgL, kp1).astype(np.int64) - oracle.extract_descriptors(imgR, kp2).astype(np.int64)
    assert np.array_equal(Sx[:, 1], np.abs(d).sum(1))              # the row's dist for a real match
    for mode in (1, 2):
        uv = S.refine(oracle, imgL, imgR, kp1, kp2, match, mode)
        assert uv.dtype == np.float32 and uv.shape == (n, 2)
        assert np.abs(uv - q).max() <= 0.5
        want_u = (q[:, 0] + S.parabola_offset(Sx[:, 0], Sx[:, 1], Sx[:, 2])).astype(np.float32)
        assert np.array_equal(uv[:, 0], want_u)
        if mode == 1:
            assert np.array_equal(uv[:, 1], q[:, 1].astype(np.float32))
        else:
            assert np.array_equal(uv[:, 1], (q[:, 1] + S.parabola_offset(Sy[:, 0], Sy[:, 1], Sy[:, 2])).astype(np.float32))


@pytest.fixture(scope="module")
def scene():
    return synth.make_subpixel_image_sequence(2, 24, n_kp=1500)


@pytest.fixture(scope="module")
def runs(oracle, scene):
    return {m: S.pipeline(oracle, scene, m, seed=3) for m in (0, 1)}


def test_mode0_assembly_is_the_oracle_sequence(oracle, scene, runs):
    from libviso_amd.abi import MatchParams
    desc = S.extract_all(oracle, scene)
    want = oracle.sequence(scene["kp"], desc, scene["n"], MatchParams.stereo(scene["F"]), MatchParams.temporal(),
                           scene["param"], seed=3)
    got = runs[0]
    assert np.array_equal(got["tr"], want["tr"]) and np.array_equal(got["ok"], want["ok"])
    assert np.array_equal(got["n_inl"], want["n_inl"])


def test_refined_disparity_is_closer_to_the_truth(scene, runs):
    # stereo rows that join two projections of one world point (same true row, integer disparity within a pixel of the truth)
    ei, er = [], []
    for t in range(scene["kp"].shape[0]):
        m, uv = runs[1]["lr"][t], runs[1]["uv"][t]
        a, b = scene["xy_true"][t, 0, m[:, 0]], scene["xy_true"][t, 1, m[:, 1]]
        kl, kr = scene["kp"][t, 0, m[:, 0]], scene["kp"][t, 1, m[:, 1]]
        dtrue = a[:, 0] - b[:, 0]
        dint = kl[:, 0].astype(np.float64) - kr[:, 0]
        good = np.isfinite(dtrue) & (a[:, 1] == b[:, 1]) & (np.abs(dint - dtrue) < 1.5)
        ei.append(np.abs(dint - dtrue)[good])
        er.append(np.abs(kl[good, 0].astype(np.float64) - uv[good, 0] - dtrue[good]))
    ei, er = np.concatenate(ei), np.concatenate(er)
    assert len(ei) > 10000
    # measured: median 0.28 px -> 0.17 px (mean 0.33 -> 0.27)
    assert np.median(er) < 0.7 * np.median(ei)
    assert er.mean() < 0.95 * ei.mean()


def test_refinement_lowers_the_translation_error(scene, runs):
    e0 = S.translation_errors(runs[0]["tr"], scene["tr_gt"])
    e1 = S.translation_errors(runs[1]["tr"], scene["tr_gt"])
    assert runs[0]["ok"][1:].all() and runs[1]["ok"][1:].all()
    # measured on this scene: median 6.1 mm -> 5.2 mm (0.85); 0.83 and 0.92 on seeds 1 and 3
    assert np.median(e1) < 0.95 * np.median(e0)
