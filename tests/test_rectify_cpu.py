"""No-GPU checks of the opt-in rectification of raw images (include/viso_hip.h, viso_rectify_map / viso_batch_set_rectify):
the host map builder against its numpy restatement (tests/rectify_ref.py), the identity calibration, argument errors, and the
device entry points failing loudly without a device."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd import synth

import rectify_ref as RR


def _random_calib(rng, strong):
    f = rng.uniform(300, 1200)
    K = np.array([[f, 0, rng.uniform(200, 800)], [0, f * rng.uniform(0.97, 1.03), rng.uniform(100, 400)], [0, 0, 1]])
    if strong:
        D = np.array([rng.uniform(-0.45, -0.25), rng.uniform(0.05, 0.3), rng.uniform(-5e-3, 5e-3), rng.uniform(-5e-3, 5e-3),
                      rng.uniform(-0.1, 0.05)])
    else:
        D = rng.uniform(-0.02, 0.02, 5)
    R = synth.rot_from_tr(np.concatenate([rng.uniform(-0.03, 0.03, 3), np.zeros(3)]))[0]
    fp = rng.uniform(300, 1000)
    P = np.array([[fp, 0, rng.uniform(100, 600), rng.uniform(-400, 0)], [0, fp, rng.uniform(50, 300), 0], [0, 0, 1, 0]])
    return K, D, R, P


def test_map_builder_matches_the_restatement():
    rng = np.random.default_rng(1)
    for rep in range(12):
        K, D, R, P = _random_calib(rng, strong=rep % 3 != 0)
        shape = (int(rng.integers(1, 300)), int(rng.integers(1, 500)))
        mx, my = libviso_amd.rectify_map(K, D, R, P, shape)
        wx, wy = RR.rectify_map(K, D, R, P, shape)
        assert mx.dtype == np.float32 and mx.shape == shape
        assert np.abs(mx.astype(np.float64) - wx).max() <= 1e-3 and np.abs(my.astype(np.float64) - wy).max() <= 1e-3, rep
    c = synth.raw_stereo_calib()
    for s in (0, 1):
        mx, my = libviso_amd.rectify_map(c["K"][s], c["D"][s], c["R"][s], c["P"][s], c["out_shape"])
        wx, wy = RR.maps_of(c)[s]
        assert np.abs(mx - wx).max() <= 1e-3 and np.abs(my - wy).max() <= 1e-3
        raw_rows, raw_cols = c["raw_shape"]   # the synthetic raw camera sees the whole rectified view
        assert mx.min() >= 0 and mx.max() <= raw_cols - 1 and my.min() >= 0 and my.max() <= raw_rows - 1


def test_identity_calibration_gives_the_pixel_grid():
    for K in (np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]]),
              np.array([[721.5377, 0, 609.5593], [0, 721.5377, 172.854], [0, 0, 1]]),
              np.array([[100.0, 0, 900.25], [0, 90.3, 1000.7], [0, 0, 1]])):
        P = np.hstack([K, [[-387.57], [0], [0]]])
        mx, my = libviso_amd.rectify_map(K, np.zeros(5), np.eye(3), P, (376, 1241))
        gy, gx = np.mgrid[0:376, 0:1241].astype(np.float32)
        assert np.array_equal(mx, gx) and np.array_equal(my, gy)


def test_quantisation_restatement_hand_cases():
    m = np.array([0.0, 0.015625, 0.046875, -0.015625, -0.03125, 1.5, -1.0, 31.99, 32767.99, 32768.0, np.nan, np.inf, -np.inf, -40000.0],
                 np.float32)
    ix, iy, fx, fy, out = RR.quantise(m, np.zeros_like(m))
    # x32: 0, 0.5 (ties to even: 0), 1.5 (2), -0.5 (-0), -1, 48, -32, 1023.68 (1024), 1048575.69 (1048576)
    assert ix[:9].tolist() == [0, 0, 0, 0, -1, 1, -1, 32, 32768] and fx[:9].tolist() == [0, 0, 2, 0, 31, 16, 0, 0, 0]
    assert out.tolist() == [False] * 9 + [True] * 5


def test_argument_errors_return_codes():
    L = libviso_amd.load()
    K, D, R, P = synth.raw_stereo_calib()["K"][0], np.zeros(5), np.eye(3), synth.KITTI_P1
    Ks = K.copy(); Ks[0, 1] = 0.5
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        libviso_amd.rectify_map(Ks, D, R, P, (10, 10))
    for shape in ((0, 10), (10, 0), (-1, 5)):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.rectify_map(K, D, R, P, shape)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        libviso_amd.rectify_map(K, D, np.zeros((3, 3)), P, (10, 10))   # P33 R singular
    mx = np.zeros((4, 5), np.float32)
    raw = np.zeros((2, 6, 7), np.uint8)
    for border in (-1, 256):
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            libviso_amd.rectify_images(raw, mx, mx, (4, 5), border=border)
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        libviso_amd.rectify_images(np.zeros((2, 0, 7), np.uint8), mx, mx, (4, 5))
    u8 = C.POINTER(C.c_uint8)
    f = C.POINTER(C.c_float)
    pm = mx.ctypes.data_as(f)
    assert L.viso_rectify_images(raw.ctypes.data_as(u8), 2, 6, 7, pm, None, 4, 5, 0, raw.ctypes.data_as(u8)) == -1
    assert L.viso_batch_set_rectify(None, 6, 7, 4, 5, pm, pm, pm, pm, 0) == -1
    assert L.viso_batch_get_image(None, 0, 0, raw.ctypes.data_as(u8)) == -1


def test_device_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    mx, my = np.meshgrid(np.arange(5, dtype=np.float32), np.arange(4, dtype=np.float32))
    with pytest.raises(libviso_amd.VisoError, match="-2"):
        libviso_amd.rectify_images(np.zeros((2, 6, 7), np.uint8), mx, my, (4, 5))


def test_distorted_scene_round_trip():
    """synth.distort_image_sequence renders raw images whose rectification restores the rectified scene up to interpolation."""
    seq = synth.make_subpixel_image_sequence(4, 2, n_kp=300, width=320, height=120)   # smooth textures: interpolation is mild
    calib = synth.raw_stereo_calib(2, raw_shape=(150, 360), out_shape=(120, 320))
    d = synth.distort_image_sequence(seq, calib, seed=3)
    assert d["images"].shape == (2, 2, 150, 360) and np.array_equal(d["images_rect"], seq["images"])
    back = RR.rectify_sequence(d["images"], RR.maps_of(calib))
    diff = np.abs(back.astype(int) - seq["images"].astype(int))
    assert np.median(diff) <= 1.5 and diff.mean() <= 3, (np.median(diff), diff.mean())   # measured: 1.0, 2.05


def test_map_builder_with_large_rotations():
    """Rotations far from a rectifying one (the elimination pivots): still the header's formula."""
    rng = np.random.default_rng(9)
    K = np.array([[700.0, 0, 600], [0, 700, 180], [0, 0, 1]])
    P = np.hstack([K, np.zeros((3, 1))])
    for rot in ([0, 0, 1.5], [0, 1.2, 0], [1.3, 0.2, 0.9], [0.1, 0.1, 3.0], [1.5, 1.5, 0.0]):
        R = synth.rot_from_tr(np.array(rot + [0, 0, 0]))[0]
        D = np.array([-0.1, 0.02, 1e-3, -1e-3, 0.0])
        mx, my = libviso_amd.rectify_map(K, D, R, P, (60, 90))
        wx, wy = RR.rectify_map(K, D, R, P, (60, 90))
        ok = (np.abs(wx) < 1e4) & (np.abs(wy) < 1e4)
        assert ok.any()
        tol = 1e-3 * np.maximum(1.0, np.maximum(np.abs(wx), np.abs(wy)) / 1e3)
        assert (np.abs(mx - wx)[ok] <= tol[ok]).all() and (np.abs(my - wy)[ok] <= tol[ok]).all(), rot
    # cx far beyond fx (the pivot is swapped): the identity is still the grid to well below the quantisation step
    K = np.array([[50.0, 0, 900.5], [0, 40.0, 700.25], [0, 0, 1]])
    mx, my = libviso_amd.rectify_map(K, np.zeros(5), np.eye(3), np.hstack([K, np.zeros((3, 1))]), (20, 30))
    gy, gx = np.mgrid[0:20, 0:30]
    assert np.abs(mx - gx).max() < 1e-3 and np.abs(my - gy).max() < 1e-3
    del rng


def test_cam_to_cam_parser(tmp_path):
    """KITTI raw calib_cam_to_cam.txt through the C++ parser of the runners (viso_kitti_load_cam_to_cam, libviso_host.so)."""
    from libviso_amd import kitti_shard
    c = synth.raw_stereo_calib(4)
    got = kitti_shard.load_cam_to_cam(RR.write_cam_to_cam(str(tmp_path / "calib_cam_to_cam.txt"), c))
    assert got["raw_shape"] == c["raw_shape"] and got["out_shape"] == c["out_shape"]
    for key in ("K", "D", "R", "P"):
        for s in (0, 1):
            assert np.array_equal(got[key][s], np.asarray(c[key][s], np.float64)), (key, s)
    for drop in ("S_00", "K_01", "D_00", "R_rect_01", "P_rect_00", "S_rect_01"):
        with pytest.raises(ValueError):
            kitti_shard.load_cam_to_cam(RR.write_cam_to_cam(str(tmp_path / f"m_{drop}.txt"), c, drop=drop))
    for extra in ("D_01", "P_rect_01", "S_00"):
        with pytest.raises(ValueError):
            kitti_shard.load_cam_to_cam(RR.write_cam_to_cam(str(tmp_path / f"e_{extra}.txt"), c, extra_value=extra))
    with pytest.raises(ValueError):
        kitti_shard.load_cam_to_cam(str(tmp_path / "absent.txt"))
    L = kitti_shard.load_host()
    assert L.viso_kitti_set_rectify(str(tmp_path / "absent.txt").encode()) == -1
    assert L.viso_kitti_set_rectify(None) == 1


def test_kitti_runner_rejects_a_bad_cam_to_cam(tmp_path):
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(libviso_amd.SO_PATH), "viso_kitti")
    os.makedirs(tmp_path / "sequences" / "00")
    env = dict(os.environ, KITTI_HOME=str(tmp_path))
    r = subprocess.run([exe, "x", "00", "--rectify", str(tmp_path / "absent.txt")], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 2 and "calib_cam_to_cam" in r.stderr
    r = subprocess.run([exe, "x", "00", "--rectify"], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 1
