"""Textured scenes for the photometric frame-to-model alignment (tests/photo_align_ref.py; tsdf_gray_linearize_kernel in
libviso_amd/csrc/tsdf_align.hip), shared by tests/test_photo_align_cpu.py, tests/test_gpu_photo_align.py and
tests/test_gpu_photo_align_tool.py.

Two analytic scenes under one smooth texture that is fixed in the world, ray cast exactly to disparity in 1/16 px and to an 8-bit
intensity: the wall, one plane n = (0, 0, 1), d = 6, on which the signed distance leaves the three motions inside the plane free,
and the room, the three planes of tests/align_cases.py.  The cameras, the guess, the calibration and the shape are align_cases'.
The texture's periods (1.7 m and 1.3 m) span several voxels of 0.1 m and of 0.2 m.  The models are fused from the three views of
align_cases.FUSED by tests/gray_ref.py.
No device and no library at module level."""
import functools
import math

import numpy as np

import align_cases as AC
import gray_ref as GR

WALL = ((np.array([0.0, 0.0, 1.0]), 6.0),)
SCENES = {"wall": WALL, "room": AC.PLANES}


def texture(Q):
    """The intensity of the world points Q [..][3], before rounding."""
    x, y, z = Q[..., 0], Q[..., 1], Q[..., 2]
    return 128.0 + 45.0 * np.sin(2.0 * math.pi * x / 1.7 + 0.9 * y) + 40.0 * np.sin(2.0 * math.pi * y / 1.3 - 0.5 * x + 0.7 * z)


def raycast(pose, scene="wall", shape=AC.SHAPE, prm=None, noise=0.0, seed=0):
    """(int16 map, uint8 image) of the scene from `pose`: per pixel the nearest plane along its ray, disp16 = floor((FB / Z) 16 + 0.5)
    and the texture at the point that the ray meets, rounded.  noise: Gaussian image noise in gray levels."""
    prm = AC.param(shape) if prm is None else prm
    rows, cols = shape
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    rays = np.stack([(x - prm.cu) / prm.f, (y - prm.cv) / prm.f, np.ones_like(x)], axis=-1)
    T = np.asarray(pose, np.float64)
    dirs, o = rays @ T[:3, :3].T, T[:3, 3]
    Z = np.full(shape, np.inf)
    for n, d in SCENES[scene]:
        with np.errstate(divide="ignore"):
            t = (d - n @ o) / (dirs @ n)
        Z = np.where(t > 0, np.minimum(Z, t), Z)
    v = np.floor((prm.f * prm.base / Z) * 16.0 + 0.5)
    assert np.isfinite(Z).all() and (v >= 16).all() and (v < 32768).all()
    g = texture(o + dirs * Z[..., None])
    if noise:
        g = g + np.random.default_rng(seed).normal(scale=noise, size=shape)
    return v.astype(np.int16), np.clip(np.floor(g + 0.5), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def model(scene="wall", voxel=0.1, trunc=3):
    """The gray entries of the scene fused from the three views of align_cases.FUSED, sorted by key; shared and not to be changed."""
    prm = AC.param()
    e, _ = GR.fuse([raycast(T, scene) + (T,) for T in AC.FUSED], prm, voxel=voxel, trunc=trunc)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def frame(scene="wall", noise=0.0):
    """(map, image) of the scene from align_cases.TRUTH; shared and not to be changed."""
    m, g = raycast(AC.TRUTH, scene, noise=noise)
    m.setflags(write=False)
    g.setflags(write=False)
    return m, g


def constant_gray(entries, level):
    """Plain or gray entries as gray entries whose every voxel has the mean intensity `level`."""
    return GR.with_gray(GR.plain(entries) if "gray" in entries.dtype.names else entries, entries["weight"].astype(np.uint64) * np.uint64(level))


def random_gray(entries, seed=4):
    """Plain entries (tests/tsdf_tables.py) as gray entries with random sums of intensities 0 .. 255 weight, a tenth each at both ends."""
    rng = np.random.default_rng(seed)
    w = entries["weight"].astype(np.int64)
    special = rng.integers(0, 10, len(w))
    return GR.with_gray(entries, np.where(special == 0, 0, np.where(special == 1, 255 * w, rng.integers(0, 255 * w + 1))))


# ---- tables built by hand ---------------------------------------------------------------------------------------------------------
def _block(kz, gray_of, half=4, weight=2):
    """(2 half)^2 x 8 voxels of weight `weight` and sum 0 (the distance and its gradient are zero everywhere: every geometric row
    is zero and every pixel with a whole cell is used), kx, ky in -half .. half - 1, kz .. kz + 7; gray_of(k [n][3]) is the mean
    intensity of each."""
    g = np.stack(np.meshgrid(np.arange(-half, half), np.arange(-half, half), np.arange(kz, kz + 8), indexing="ij"), axis=-1).reshape(-1, 3)
    e = np.zeros(len(g), GR.ENTRY)
    e["k"], e["weight"] = g, weight
    e["gray"] = gray_of(g).astype(np.uint64) * np.uint64(weight)
    return e[np.argsort(GR.keys_of(e["k"]))]


def clip_case():
    """(entries, voxel, map, image, param) in which P5 ends some photometric rows and not all, at the default lambda = 1 / 32.  The
    block lies 100 m ahead (1 px of disparity, a pixel is 0.01 m there).  Above the axis (ky < 0) the intensity alternates between 0
    and 255 from voxel to voxel along y: 2550 gray levels per metre, and the lever of 100 m makes b_3 = Z hc_1 lambda = 7969 >= 4096.
    Below it the intensity is 100 everywhere: the row is (0, .., 0, r lambda), which fits."""
    prm = AC.Param.default(base=0.01, f=10000.0, cu=39.5, cv=19.5)
    e = _block(996, lambda k: np.where(k[:, 1] < 0, np.where(k[:, 1] & 1, 255, 0), 100))
    return e, 0.1, np.full((40, 80), 16, np.int16), np.full((40, 80), 90, np.uint8), prm


def one_run_case():
    """(entries, voxel, map, image, param): two rows of 64 pixels, each a whole wave whose 64 points lie in one cell, (-1, -1, 99):
    the block 10 m ahead under a pixel of 0.001 m, with a random intensity per voxel."""
    prm = AC.Param.default(base=0.001, f=10000.0, cu=31.5, cv=0.5)
    rng = np.random.default_rng(6)
    e = _block(96, lambda k: rng.integers(0, 256, len(k)))
    image = rng.integers(0, 256, (2, 64)).astype(np.uint8)
    return e, 0.1, np.full((2, 64), 16, np.int16), image, prm
