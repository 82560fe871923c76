"""Random differential tests of the dense image stage on the device (tests/dense_fuzz.py): every direct call once per case against
its numpy restatement, exact (np.array_equal; the points bit for bit), and one resident batch past the remap's 32-frame chunk.
tests/test_dense_fuzz_cpu.py checks, on the restatements alone, that these seeds and counts reach the launch seams.

The counts are sized by the restatements, about 5 s a test function at the most.  Measured on one CPU core of the build machine,
per seed (dense_fuzz.COUNTS):
    stereo_disparity     150 cases   4.3 - 5.2 s   (disparity_ref.disparity)
    stereo_sgm           160 cases   3.6 - 4.7 s   (sgm_ref.sgm)
    filter_speckles      300 cases   0.1 s         (speckle_ref.speckles; drawing the cases, which sizes the components, 0.2 s)
    rectify_images       100 cases   0.6 - 0.7 s   (rectify_ref.remap, a call per frame)
    disparity_to_points  150 cases   0.04 s        (speckle_ref.points)
    the resident batch   33 / 65 frames of 24 x 40: 0.2 s / 0.9 s
The device side of a case is a launch or a few and three small copies.

A failing case prints dense_fuzz.describe(case): kind, seed and index are enough to draw it again,
    next(itertools.islice(dense_fuzz.CASES[kind](seed, index + 1), index, None))
A seed that finds something is pinned here with the case and what it found.  None so far: seeds 0 .. 2 agree with the restatements
everywhere, and so does the sweep `python3 tests/dense_fuzz.py 0 2000` (2000 cases of each of the five calls, 0 mismatches, 56 s on
an MI355X host).  That the comparison bites was checked once by hand with a library carrying five value-only changes (<= for < at
the block matcher's new best, no path restart at the right image edge in SGM, < for <= at the speckle size, > for >= at min_disp16,
the remap reading frame f % 32): every test function of this file failed, within its first ten cases."""
import numpy as np
import pytest

import libviso_amd

import dense_fuzz as F
import disparity_ref as DR
import rectify_ref as RR
import sgm_ref as SR
import speckle_ref as K

pytestmark = pytest.mark.gpu


def _run(kind, seed):
    n = 0
    for case in F.CASES[kind](seed, F.COUNTS[kind]):
        got, want = F.device(case), F.expected(case)
        assert got.shape == want.shape and F.same(case, got, want), F.describe(case)
        n += 1
    assert n == F.COUNTS[kind]


@pytest.mark.parametrize("seed", F.SEEDS)
def test_stereo_disparity(viso, seed):
    _run("bm", seed)


@pytest.mark.parametrize("seed", F.SEEDS)
def test_stereo_sgm(viso, seed):
    _run("sgm", seed)


@pytest.mark.parametrize("seed", F.SEEDS)
def test_filter_speckles(viso, seed):
    _run("speckle", seed)


@pytest.mark.parametrize("seed", F.SEEDS)
def test_rectify_images(viso, seed):
    _run("rectify", seed)


@pytest.mark.parametrize("seed", F.SEEDS)
def test_disparity_to_points(viso, seed):
    _run("points", seed)


BATCH = {
    33: ("bm", dict(num_disp=32, block=7, prefilter_cap=63, texture_threshold=1, uniqueness=3, lr_max_diff=2)),
    65: ("sgm", dict(num_disp=48, p1=3, p2=40, paths=8, uniqueness=2, lr_max_diff=2)),
}
SPECKLE = dict(max_size=4, max_diff=24)


@pytest.mark.parametrize("nf", sorted(BATCH))
def test_resident_batch_past_the_frame_chunk(viso, nf):
    """Rectification, a dense method and the speckle filter over nf resident frames: rectify_remap_kernel walks a second (33) and a
    third (65) chunk of 32 frames, one of them partial, and the methods and the filter go through their workspace in several groups.
    Every frame's images and map against the restatement chain."""
    method, prm = BATCH[nf]
    raw_shape, out_shape, border = (30, 44), (24, 40), 91
    rng = np.random.default_rng(1000 + nf)
    maps = [F.hostile_map(rng, raw_shape, out_shape) for _ in range(2)]
    # random texture, the right camera's shifted; the hostile maps scramble it, and the methods still leave a mixed map per frame
    base = rng.integers(0, 256, (nf,) + (raw_shape[0], raw_shape[1] + 5), dtype=np.uint8)
    raw = np.ascontiguousarray(np.stack([base[:, :, 5:], base[:, :, :-5]], 1))
    assert nf > F.RECT_FPB and raw.shape == (nf, 2) + raw_shape
    ctx = libviso_amd.Context(0)
    b = libviso_amd.Batch(ctx, nf, 64)
    try:
        libviso_amd.sgm_set_workspace_cap(9 * libviso_amd.sgm_frame_bytes(*out_shape, prm["num_disp"]))
        libviso_amd.speckle_set_workspace_cap(14 * libviso_amd.speckle_frame_bytes(*out_shape))
        b.set_rectify(raw_shape, out_shape, left=maps[0], right=maps[1], border=border)
        if method == "bm":
            b.set_disparity(prm)
        else:
            b.set_sgm(prm)
        b.set_speckle(SPECKLE)
        b.upload_images_only(raw)
        b.run_disparity()
        assert b.image_shape() == out_shape
        all_d = b.disparities()
        kept = removed = 0
        for t in range(nf):
            img = [RR.remap(raw[t, s], maps[s][0], maps[s][1], border) for s in (0, 1)]
            for s in (0, 1):
                assert np.array_equal(b.image(t, s), img[s]), (nf, t, s)
            d = DR.disparity(img[0], img[1], **prm) if method == "bm" else SR.sgm(img[0], img[1], **prm)
            want = K.speckles(d, SPECKLE["max_size"], SPECKLE["max_diff"])
            assert np.array_equal(b.disparity(t), want) and np.array_equal(all_d[t], want), (nf, method, t)
            kept += int((want != K.INVALID).sum())
            removed += int((want != d).sum())
        assert kept > 0 and removed > 0   # the chain had something to decide
    finally:
        libviso_amd.sgm_set_workspace_cap(0)
        libviso_amd.speckle_set_workspace_cap(0)
        b.close(); ctx.close()


def _one_step_outside():
    """(call, bad parameters) one step past every bound the generators draw up to."""
    d_lo, d_hi = F.NUM_DISPS[0], F.NUM_DISPS[-1]
    b_lo, b_hi = F.BLOCKS[0], F.BLOCKS[-1]
    bm = [dict(num_disp=d_lo - 16), dict(num_disp=d_hi + 16), dict(num_disp=d_lo + 1), dict(num_disp=d_hi - 1),
          dict(block=b_lo - 2), dict(block=b_hi + 2), dict(block=b_lo + 1), dict(block=b_hi - 1),
          dict(prefilter_cap=F.CAP_RANGE[0] - 1), dict(prefilter_cap=F.CAP_RANGE[1] + 1), dict(texture_threshold=-1),
          dict(uniqueness=F.UNIQ_RANGE[0] - 1), dict(uniqueness=F.UNIQ_RANGE[1] + 1)]
    sgm = [dict(num_disp=d_lo - 16), dict(num_disp=d_hi + 16), dict(num_disp=d_lo + 1), dict(num_disp=d_hi - 1),
           dict(p1=F.P_RANGE[0] - 1), dict(p2=F.P_RANGE[1] + 1), dict(p1=F.P_RANGE[1] + 1, p2=F.P_RANGE[1] + 1), dict(p1=50, p2=49),
           dict(p1=F.P_RANGE[1], p2=F.P_RANGE[1] - 1),
           dict(uniqueness=F.UNIQ_RANGE[0] - 1), dict(uniqueness=F.UNIQ_RANGE[1] + 1)]
    sgm += [dict(paths=p) for p in range(F.PATHS[0] - 1, F.PATHS[1] + 2) if p not in F.PATHS]
    for D in (d_lo, 128, d_hi):   # lr_max_diff runs from -1 to num_disp
        bm += [dict(num_disp=D, lr_max_diff=-2), dict(num_disp=D, lr_max_diff=D + 1)]
        sgm += [dict(num_disp=D, lr_max_diff=-2), dict(num_disp=D, lr_max_diff=D + 1)]
    spk = [dict(max_size=-1), dict(max_diff=F.MAX_DIFF_RANGE[0] - 1), dict(max_diff=F.MAX_DIFF_RANGE[1] + 1)]
    return bm, sgm, spk


def test_parameter_checks_end_where_the_fuzz_ends(viso):
    """The generators draw up to the bounds of disparity_params_ok, sgm_params_ok and speckle_params_ok; one step past each of them
    the calls refuse (VISO_ERR_ARG), and at each of them they run.  If a check moves, this fails before the fuzz goes blind."""
    img = np.zeros((24, 40), np.uint8)
    m = np.zeros((8, 40), np.int16)
    bm, sgm, spk = _one_step_outside()
    for call, first, bads in ((libviso_amd.stereo_disparity, (img, img), bm), (libviso_amd.stereo_sgm, (img, img), sgm),
                              (libviso_amd.filter_speckles, (m,), spk)):
        for bad in bads:
            with pytest.raises(libviso_amd.VisoError, match="-1"):
                call(*first, **bad)
    mx, my = F.hostile_map(np.random.default_rng(0), (8, 40), (6, 10))
    for border in (F.BORDER_RANGE[0] - 1, F.BORDER_RANGE[1] + 1):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.rectify_images(img[:8], mx, my, (6, 10), border=border)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        libviso_amd.disparity_to_points(m, F._calib(dict(calib=dict(base=0.5, f=700.0, cu=20.0, cv=4.0))), min_disp16=0)
    # the bounds themselves are inside
    ends = [dict(num_disp=F.NUM_DISPS[0], block=F.BLOCKS[0], prefilter_cap=F.CAP_RANGE[0], texture_threshold=0,
                 uniqueness=F.UNIQ_RANGE[0], lr_max_diff=-1),
            dict(num_disp=F.NUM_DISPS[-1], block=F.BLOCKS[-1], prefilter_cap=F.CAP_RANGE[1], texture_threshold=F.TEX_HUGE,
                 uniqueness=F.UNIQ_RANGE[1], lr_max_diff=F.NUM_DISPS[-1])]
    for p in ends:
        assert np.array_equal(libviso_amd.stereo_disparity(img, img, **p), DR.disparity(img, img, **p))
    for p in (dict(num_disp=F.NUM_DISPS[0], p1=F.P_RANGE[0], p2=F.P_RANGE[0], paths=F.PATHS[0], uniqueness=F.UNIQ_RANGE[0], lr_max_diff=-1),
              dict(num_disp=F.NUM_DISPS[-1], p1=F.P_RANGE[1], p2=F.P_RANGE[1], paths=F.PATHS[1], uniqueness=F.UNIQ_RANGE[1],
                   lr_max_diff=F.NUM_DISPS[-1])):
        assert np.array_equal(libviso_amd.stereo_sgm(img, img, **p), SR.sgm(img, img, **p))
    for p in (dict(max_size=0, max_diff=F.MAX_DIFF_RANGE[0]), dict(max_size=m.size, max_diff=F.MAX_DIFF_RANGE[1])):
        assert np.array_equal(libviso_amd.filter_speckles(m, **p), K.speckles(m, p["max_size"], p["max_diff"]))
