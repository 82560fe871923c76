"""No-GPU checks of the opt-in dense stereo disparity (include/viso_hip.h, "dense stereo disparity"): the numpy restatement
against a literal per-pixel reading of the definition across the parameter edges, integer shifts, the accuracy on a slanted
textured plane, the texture, uniqueness and left-right rules on built cases, the largest cost, argument errors, the kernel's
resource usage and the device entry points failing loudly without a device."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd

import disparity_ref as DR
from estimator_util import kernel_resources

EDGES = [dict(), dict(uniqueness=0, lr_max_diff=-1), dict(uniqueness=100, lr_max_diff=0), dict(prefilter_cap=1, texture_threshold=0),
         dict(prefilter_cap=63, texture_threshold=400, uniqueness=1, lr_max_diff=16), dict(lr_max_diff=1, uniqueness=50, texture_threshold=1)]


@pytest.mark.parametrize("block", [5, 7])
@pytest.mark.parametrize("edge", range(len(EDGES)))
def test_restatement_equals_the_literal_loop(block, edge):
    rng = np.random.default_rng(10 * block + edge)
    L = rng.integers(0, 256, (20, 48)).astype(np.uint8)
    R = np.roll(L, -(edge % 5 + 1), axis=1)
    R[:, ::7] = rng.integers(0, 256, R[:, ::7].shape)   # some disagreement so every rule has work
    for right in (R, rng.integers(0, 256, L.shape).astype(np.uint8)):
        a = DR.disparity(L, right, num_disp=16, block=block, **EDGES[edge])
        b = DR.disparity_loop(L, right, num_disp=16, block=block, **EDGES[edge])
        assert np.array_equal(a, b)


def test_small_geometries_are_all_invalid():
    rng = np.random.default_rng(2)
    for shape in ((10, 48), (20, 10), (4, 4)):
        L = rng.integers(0, 256, shape).astype(np.uint8)
        assert (DR.disparity(L, L, block=11) == DR.INVALID).all()
    L = rng.integers(0, 256, (11, 11)).astype(np.uint8)
    d = DR.disparity(L, L, block=11, texture_threshold=0)
    assert d[5, 5] == 0 and (d != DR.INVALID).sum() == 1


@pytest.mark.parametrize("shift", [0, 3, 17])
def test_integer_shift_gives_sixteen_d(shift):
    """d* is exact at every textured interior pixel; the V-fit moves the output by less than half a pixel (p != n in general)."""
    rng = np.random.default_rng(shift)
    base = rng.integers(0, 256, (40, 160 + shift)).astype(np.uint8)
    L, R = np.ascontiguousarray(base[:, :160]), np.ascontiguousarray(base[:, shift:])   # R(x - shift) = L(x)
    for sub in (False, True):
        d = DR.disparity(L, R, subpixel=sub, num_disp=32, block=7)
        core = d[3:-3, shift + 3:-3]
        ok = core[core != DR.INVALID]
        assert ok.size > 0.95 * core.size
        if sub:
            assert (np.abs(ok.astype(int) - 16 * shift) <= 8).all()
        else:
            assert (ok == 16 * shift).all()


def test_slanted_plane_accuracy():
    L, R, dtrue = DR.slanted_pair()
    valid, med, big = DR.accuracy(DR.disparity(L, R), dtrue)
    _, med0, _ = DR.accuracy(DR.disparity(L, R, subpixel=False), dtrue)
    print(f"valid {valid:.3f} median {med:.3f} px (no sub-pixel {med0:.3f}) > 1 px {big:.4f}")
    assert valid >= 0.85 and med <= 0.12 and big <= 0.01 and med < med0


def test_flat_image_is_all_invalid_with_a_texture_threshold():
    L = np.full((40, 80), 77, np.uint8)
    assert (DR.disparity(L, L, num_disp=16, texture_threshold=1) == DR.INVALID).all()
    d = DR.disparity(L, L, num_disp=16, texture_threshold=0, uniqueness=0, lr_max_diff=-1)
    assert (d[5:-5, 5:-5] == 0).all()


def test_periodic_texture_is_rejected_by_uniqueness():
    x = np.arange(200)
    row = (128 + 100 * np.sin(2 * np.pi * x / 8)).astype(np.uint8)
    L = np.tile(row, (30, 1))
    R = np.roll(L, -3, axis=1)
    on = DR.disparity(L, R, num_disp=32, block=7, uniqueness=15, lr_max_diff=-1)
    off = DR.disparity(L, R, num_disp=32, block=7, uniqueness=0, lr_max_diff=-1)
    assert (on[3:-3, 40:-10] == DR.INVALID).all()
    assert (off[3:-3, 40:-10] != DR.INVALID).all()


def test_occluding_step_is_cut_by_the_lr_check():
    rng = np.random.default_rng(5)
    rows, cols, dfg, dbg = 40, 200, 20, 4
    bg = rng.integers(0, 256, (rows, cols + 64)).astype(np.uint8)
    fg = rng.integers(0, 256, (rows, cols + 64)).astype(np.uint8)
    xs = np.arange(cols)
    L = np.where(xs[None, :] >= 100, fg[:, xs], bg[:, xs]).astype(np.uint8)
    # right image: background shifted by dbg, the foreground (x >= 100 in the left) by dfg: it covers right columns >= 100 - dfg
    R = np.where(xs[None, :] >= 100 - dfg, fg[:, xs + dfg], bg[:, xs + dbg]).astype(np.uint8)
    on = DR.disparity(L, R, num_disp=32, block=7, uniqueness=0, lr_max_diff=1)
    off = DR.disparity(L, R, num_disp=32, block=7, uniqueness=0, lr_max_diff=-1)
    band = slice(100 - dfg + dbg + 4, 100 - 4)   # left background pixels whose right partners the foreground hides
    assert (on[5:-5, band] == DR.INVALID).mean() > 0.8
    assert (off[5:-5, band] != DR.INVALID).mean() > 0.9


def largest_cost_pair():
    """0/255 columns in pairs: P_L is 0 or 126 at every interior pixel (c = 63), and the inverted right image has P_R = 126 - P_L."""
    x = np.arange(64)
    L = np.tile(np.where((x // 2) % 2 == 0, 0, 255), (30, 1)).astype(np.uint8)
    return L, (255 - L).astype(np.uint8)


def test_largest_cost_is_reached():
    L, R = largest_cost_pair()
    PL, PR = DR.prefilter(L, 63).astype(np.int64), DR.prefilter(R, 63).astype(np.int64)
    assert set(np.unique(PL[:, 1:-1])) == {0, 126} and (PR[:, 1:-1] == 126 - PL[:, 1:-1]).all()
    C = DR._cost(PL, PR, 0, 10)
    assert C.max() == 2 * 63 * 21 * 21 == 55566


def test_argument_errors_return_codes():
    L = libviso_amd.load()
    img = np.zeros((30, 40), np.uint8)
    out = np.zeros((30, 40), np.int16)
    u8, i16 = C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
    good = libviso_amd.disparity_params()
    assert (good.num_disp, good.block, good.prefilter_cap, good.texture_threshold, good.uniqueness, good.lr_max_diff) == (
        128, 11, 31, 10, 15, 1)
    bad = [dict(num_disp=0), dict(num_disp=8), dict(num_disp=24), dict(num_disp=272), dict(block=4), dict(block=3), dict(block=23),
           dict(block=12), dict(prefilter_cap=0), dict(prefilter_cap=64), dict(texture_threshold=-1), dict(uniqueness=-1),
           dict(uniqueness=101), dict(lr_max_diff=-2), dict(num_disp=16, lr_max_diff=17)]
    for b in bad:
        p = libviso_amd.disparity_params(**b)
        assert L.viso_stereo_disparity(img.ctypes.data_as(u8), img.ctypes.data_as(u8), 30, 40, C.byref(p), out.ctypes.data_as(i16)) == -1, b
        assert L.viso_batch_set_disparity(None, C.byref(p)) == -1
    for edge in (dict(num_disp=256, lr_max_diff=256), dict(num_disp=16, lr_max_diff=16), dict(block=21, prefilter_cap=63),
                 dict(block=5, prefilter_cap=1, uniqueness=100, lr_max_diff=-1)):
        assert DR.check_params(**dict(DR.DEFAULTS, **edge))
    args = [img.ctypes.data_as(u8), img.ctypes.data_as(u8), 30, 40, C.byref(good), out.ctypes.data_as(i16)]
    for i, v in ((0, None), (1, None), (2, 0), (3, 0), (2, -1), (4, None), (5, None)):
        a = list(args)
        a[i] = v
        assert L.viso_stereo_disparity(*a) == -1, i
    wide = np.zeros((8, 2049), np.uint8)
    wout = np.zeros((8, 2049), np.int16)
    assert L.viso_stereo_disparity(wide.ctypes.data_as(u8), wide.ctypes.data_as(u8), 8, 2049, C.byref(good), wout.ctypes.data_as(i16)) == -3
    assert L.viso_batch_set_disparity(None, None) == -1
    assert L.viso_batch_run_disparity(None) == -1
    assert L.viso_batch_get_disparity(None, 0, out.ctypes.data_as(i16)) == -1
    assert L.viso_batch_get_disparities(None, out.ctypes.data_as(i16)) == -1
    with pytest.raises(TypeError):
        libviso_amd.disparity_params(speckle=1)
    with pytest.raises(ValueError):
        libviso_amd.stereo_disparity(img, img[:, :-1])


def test_disparity_to_float():
    d = np.array([[-16, 0, 16, 1000]], np.int16)
    f = libviso_amd.disparity_to_float(d)
    assert f.dtype == np.float32 and np.isnan(f[0, 0]) and list(f[0, 1:]) == [0.0, 1.0, 62.5]


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (376, 1241), (200, 400)])
def test_png_writer_round_trips(tmp_path, shape):
    """viso_write_disparity_png (libviso_host.so, no device): decoded with Python's zlib it gives 16 * disp16 and 0 where invalid;
    376 x 1241 and 200 x 400 span several stored blocks (65 535 bytes each)."""
    from libviso_amd.kitti_shard import load_host
    H = load_host()
    rng = np.random.default_rng(shape[0])
    d = rng.integers(0, 16 * 256, shape).astype(np.int16)
    d[rng.random(shape) < 0.3] = DR.INVALID
    d.flat[0] = 0
    f = str(tmp_path / "d.png")
    assert H.viso_write_disparity_png(f.encode(), d.ctypes.data_as(C.POINTER(C.c_int16)), shape[0], shape[1]) == 1
    got = DR.read_disparity_png(f)
    assert got.shape == shape and np.array_equal(got, DR.kitti_png_values(d))
    size = __import__("os").path.getsize(f)
    assert size < (2 * shape[1] + 1) * shape[0] * 1.01 + 100
    for args in ((None, d.ctypes.data_as(C.POINTER(C.c_int16)), 2, 2), (f.encode(), None, 2, 2), (f.encode(), d.ctypes.data_as(C.POINTER(C.c_int16)), 0, 2),
                 (str(tmp_path / "no" / "such" / "d.png").encode(), d.ctypes.data_as(C.POINTER(C.c_int16)), 1, 1)):
        assert H.viso_write_disparity_png(*args) == -1


def test_kitti_set_disparity_checks_its_arguments(tmp_path):
    from libviso_amd.kitti_shard import load_host
    H = load_host()
    assert H.viso_kitti_set_disparity(None, None) == 1 and H.viso_kitti_set_disparity(b"", None) == 1   # off
    bad = libviso_amd.disparity_params(block=4)
    assert H.viso_kitti_set_disparity(str(tmp_path / "d").encode(), C.addressof(bad)) == -1
    good = libviso_amd.disparity_params(num_disp=64)
    assert H.viso_kitti_set_disparity(str(tmp_path / "d").encode(), C.addressof(good)) == 1
    assert (tmp_path / "d").is_dir()
    assert H.viso_kitti_set_disparity(None, None) == 1


def test_kernel_has_no_scratch():
    res = kernel_resources("disparity.hip", ("stereo_disparity_kernel",))
    for name, (occ, scratch) in res.items():
        print(f"{name}: occupancy {occ}, scratch {scratch}")
        assert scratch == 0 and occ >= 1


def test_device_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    img = np.zeros((30, 40), np.uint8)
    with pytest.raises(libviso_amd.VisoError, match="-2"):
        libviso_amd.stereo_disparity(img, img)
