"""The known answers of the gray TSDF map, shared by tests/test_gray_cpu.py (on the restatement) and tests/test_gpu_gray.py (on the
device): walls of constant disparity seen and rendered from one pose, and what intensity may come back from them.  No device and no
library at module level."""
import math

import numpy as np

from libviso_amd import hostmath
from libviso_amd.abi import Param

INVALID = -16
POSE = np.linalg.inv(hostmath.tr2mat([0.013, -0.021, 0.007, 0.31, -0.12, 1.47]))   # the pose of test_gpu_tsdf
SHAPE = (40, 130)
TRUNC = 3
# name: (disparity in 1/16 px, voxel, how far a ray is followed)
WALLS = {"d400": (400, 0.2, 20.0), "d160": (160, 0.2, 40.0), "d900": (900, 0.05, 8.0)}
POSES = {"none": None, "rigid": POSE}
CASES = [(w, p) for w in WALLS for p in POSES]


def param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)   # test_gpu_tsdf's: non-integer cu, cv


def wall(name):
    """(int16 map, voxel, max_depth, depth Z of the wall in metres)."""
    d16, voxel, max_depth = WALLS[name]
    prm = param()
    return np.full(SHAPE, d16, np.int16), voxel, max_depth, prm.f * prm.base / (d16 / 16.0)


def images():
    """name: uint8 image of SHAPE.  const: 137 everywhere; ramp: 1 gray a pixel along the row; random: with 0 and 255 in it."""
    rows, cols = SHAPE
    rnd = np.random.default_rng(77).integers(0, 256, SHAPE).astype(np.uint8)
    rnd.flat[0], rnd.flat[-1] = 0, 255
    return {"const": np.full(SHAPE, 137, np.uint8), "ramp": np.tile((60 + np.arange(cols)).astype(np.uint8), (rows, 1)), "random": rnd}


def window(name):
    """w: a rendered pixel's intensity lies between the smallest and the largest intensity of the image within +-w px of it.
    A voxel's mean is a mean of the pixels whose rays crossed it, the interpolation of two means lies between them, and a ray that
    crosses a voxel the pixel's own ray crosses is at most the voxel's diagonal voxel sqrt(3) away from it, at a depth of at least
    Z - 4 voxel (the band of T = 3 voxels and the voxel itself): f voxel sqrt(3) / (Z - 4 voxel) px, rounded up, and one more for
    the rounding of the pixel's own position."""
    _, voxel, _, Z = wall(name)
    return math.ceil(param().f * voxel * math.sqrt(3.0) / (Z - 4.0 * voxel)) + 1


def window_bounds(image, w):
    """(lo, hi) int [rows][cols]: the smallest and the largest intensity within +-w px (the image's border clips the window)."""
    rows, cols = image.shape
    lo, hi = np.zeros(image.shape, np.int64), np.zeros(image.shape, np.int64)
    for y in range(rows):
        for x in range(cols):
            win = image[max(0, y - w):y + w + 1, max(0, x - w):x + w + 1]
            lo[y, x], hi[y, x] = win.min(), win.max()
    return lo, hi


def check_render(tag, image, w, d16, gray):
    """The known answers of one rendered view of a wall fused from `image`; prints the largest |g - I| over the valid pixels."""
    valid = d16 != INVALID
    assert valid.any(), tag
    assert (gray[~valid] == 0).all(), tag
    lo, hi = window_bounds(image, w)
    g = gray.astype(np.int64)
    worst = int(np.abs(g - image.astype(np.int64))[valid].max())
    inside = (g >= lo) & (g <= hi)
    print(f"{tag}: {int(valid.sum())} valid pixels, window +-{w} px, largest |g - I| = {worst}, inside the window {100.0 * inside[valid].mean():.1f} %")
    assert inside[valid].all(), tag
    return worst
