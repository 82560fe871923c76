"""Scenes and tables for the frame-to-model alignment (tests/align_ref.py; tsdf_linearize_kernel in libviso_amd/csrc/tsdf_align.hip),
shared by tests/test_align_cpu.py, tests/test_gpu_align.py and tests/test_gpu_align_tool.py.

The scene is analytic: the inside of a convex room of three planes, each at 25 degrees of incidence to the first view's axis (no
wall is nearer than 60 degrees to the axis of any view here), ray cast exactly to disparity in 1/16 px.  The three normals are
linearly independent, so all six degrees of freedom are held.  The models are fused from three views by tests/tsdf_ref.py.
The tables that are no fused scene come from tests/tsdf_tables.py (random_block).
No device and no library at module level."""
import functools
import math

import numpy as np

from libviso_amd import hostmath
from libviso_amd.abi import Param

import tsdf_ref as R
import tsdf_tables as TT

FB = 388.8                      # f base of every view: 180 x 2.16, KITTI's
SHAPE = (120, 200)
_S, _C = math.sin(math.radians(25.0)), math.cos(math.radians(25.0))
PLANES = ((np.array([_S, 0.0, _C]), 6.0), (np.array([-_S, 0.0, _C]), 6.0), (np.array([0.0, _S, _C]), 5.5))   # n . Q = d, the camera at n . Q < d


def param(shape=SHAPE):
    """The calibration of a view of `shape`: the principal point at its centre, the focal length 0.9 cols (at least 50) and the base
    that keeps f base = FB.  (120, 200): f 180, base 2.16."""
    rows, cols = shape
    f = max(0.9 * cols, 50.0)
    return Param.default(base=FB / f, f=f, cu=(cols - 1) / 2.0, cv=(rows - 1) / 2.0)


def view(rx=0.0, ry=0.0, rz=0.0, tx=0.0, ty=0.0, tz=0.0):
    """A camera-to-world pose from three angles (rad) and a position (m)."""
    T = np.linalg.inv(hostmath.tr2mat([rx, ry, rz, 0.0, 0.0, 0.0]))
    T[:3, 3] = tx, ty, tz
    return T


FUSED = (view(), view(0.010, -0.020, 0.004, 0.15, -0.05, 0.10), view(-0.012, 0.018, -0.006, -0.12, 0.06, 0.22))
TRUTH = view(0.006, 0.011, 0.003, 0.05, 0.02, 0.30)            # the fourth view
_OFF = hostmath.tr2mat([0.0045, -0.0050, 0.0040, 0.05, -0.04, 0.054])   # 0.45 degrees and 0.084 m
GUESS = TRUTH @ _OFF


def raycast(pose, shape=SHAPE, prm=None):
    """The scene from `pose` as an int16 map: per pixel the nearest plane along its ray, disp16 = floor((FB / Z) 16 + 0.5)."""
    prm = param(shape) if prm is None else prm
    rows, cols = shape
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    rays = np.stack([(x - prm.cu) / prm.f, (y - prm.cv) / prm.f, np.ones_like(x)], axis=-1)
    T = np.asarray(pose, np.float64)
    dirs, o = rays @ T[:3, :3].T, T[:3, 3]
    Z = np.full(shape, np.inf)
    for n, d in PLANES:
        with np.errstate(divide="ignore"):
            t = (d - n @ o) / (dirs @ n)
        Z = np.where(t > 0, np.minimum(Z, t), Z)
    v = np.floor((prm.f * prm.base / Z) * 16.0 + 0.5)
    assert np.isfinite(Z).all() and (v >= 16).all() and (v < 32768).all()
    return v.astype(np.int16)


@functools.lru_cache(maxsize=None)
def model(voxel=0.1, trunc=3, n_views=3):
    """The entries of the scene fused from the first n_views of FUSED, sorted by key; shared and not to be changed."""
    prm = param()
    e, _ = R.fuse([(raycast(T), T) for T in FUSED[:n_views]], prm, voxel=voxel, trunc=trunc)
    e.setflags(write=False)
    return e


def perturbed(pose, angle=0.004, shift=0.03):
    """`pose` moved by a small rigid motion on the camera's side."""
    return np.asarray(pose) @ hostmath.tr2mat([angle, -0.6 * angle, 0.4 * angle, shift, -0.5 * shift, 0.7 * shift])


# ---- maps that look into a random block (tests/tsdf_tables.py) -----------------------------------------------------------------
BLOCK_PARAM = TT.param(100.0, 99.5, 11.5)      # f base = 53.71
BLOCK_SHAPE = (24, 200)


def block_map(seed=1):
    """A map whose points lie between 0.5 m and 2.3 m: smooth on the left, so that neighbouring pixels share a cell, with noise on
    the right, so that they do not; a band of invalid pixels and one of disparities below the map's min_disp16."""
    rng = np.random.default_rng(seed)
    rows, cols = BLOCK_SHAPE
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    Z = 1.4 + 0.9 * np.sin(x / 17.0) * np.cos(y / 5.0)
    Z = np.where(x >= cols // 2, Z + rng.uniform(-0.25, 0.25, Z.shape), Z)
    d = np.floor(BLOCK_PARAM.f * BLOCK_PARAM.base / np.clip(Z, 0.4, 2.5) * 16.0 + 0.5).astype(np.int16)
    d[5, 20:60] = R.INVALID
    d[7, 100:140] = 9
    return d


def block(name="far"):
    seed, n, origin, occupancy = TT.BLOCKS[name][:4]
    return TT.random_block(np.random.default_rng(seed), n=n, origin=origin, occupancy=occupancy)


def wide_param(shape):
    """A view of `shape` that sees 35 degrees to each side where the fused views see 29: its borders look past the model."""
    rows, cols = shape
    f = 0.7 * cols if cols > 1 else 50.0
    return Param.default(base=FB / f, f=f, cu=(cols - 1) / 2.0, cv=(rows - 1) / 2.0)


CLOSE = view(tz=5.8)            # 0.27 m before the third plane: w = f base / Z^2 > 4096, the rows' limit


def usable_cells(entries, min_weight):
    """k0 [n][3] of the cells whose eight voxels are all in `entries` with weight >= min_weight."""
    e = entries[entries["weight"] >= min_weight]
    keys = R.keys_of(e["k"])
    k0 = e["k"].astype(np.int64)
    ok = np.ones(len(e), bool)
    for c in range(1, 8):
        ok &= np.isin(R.keys_of(k0 + np.array([c & 1, (c >> 1) & 1, c >> 2])), keys)
    return k0[ok]


def aim(m, cells, voxel, prm, pose=None, seed=2):
    """`m` with one pixel aimed into each of `cells` (those whose pixel is inside the image), at a random place of the cell; returns
    the number of pixels set."""
    rng = np.random.default_rng(seed)
    T = np.eye(4) if pose is None else np.asarray(pose, np.float64)
    Q = (cells + 0.5 + rng.uniform(0.2, 0.8, cells.shape)) * voxel
    P = (Q - T[:3, 3]) @ T[:3, :3]
    n = 0
    for X, Y, Z in P:
        if Z < 0.3:
            continue
        x, y = int(round(prm.f * X / Z + prm.cu)), int(round(prm.f * Y / Z + prm.cv))
        d16 = int(round(prm.f * prm.base / Z * 16.0))
        if 0 <= x < m.shape[1] and 0 <= y < m.shape[0] and 16 <= d16 < 32768:
            m[y, x] = d16
            n += 1
    return n


@functools.lru_cache(maxsize=None)
def big_block():
    """64^3 voxels at 70 % occupancy with weights 1..3: a cell with eight voxels of weight 3 has the probability (0.7 / 3)^8, so it
    takes a quarter of a million cells to hold a few.  Shared and not to be changed."""
    e = TT.random_block(np.random.default_rng(7), n=64, origin=(-32, -32, 2), occupancy=0.7)
    e.setflags(write=False)
    return e


def small_block():
    """10^3 voxels at 70 % occupancy: about 700 for a table of 2^10 slots."""
    return TT.random_block(np.random.default_rng(11), n=10, origin=(-5, -5, 3), occupancy=0.7)


def before(cell, voxel, distance=1.5):
    """The pose without rotation from which `cell` lies `distance` metres ahead on the axis."""
    T = np.eye(4)
    T[:3, 3] = (np.asarray(cell, np.float64) + 1.0) * voxel - np.array([0.0, 0.0, distance])
    return T


# ---- stereo pairs of the scene, for the maps a batch computes itself ------------------------------------------------------------
def disparity_exact(pose, shape, prm):
    """The scene's disparity in pixels at every pixel of the view, as float64 (what raycast rounds)."""
    rows, cols = shape
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    rays = np.stack([(x - prm.cu) / prm.f, (y - prm.cv) / prm.f, np.ones_like(x)], axis=-1)
    T = np.asarray(pose, np.float64)
    dirs, o = rays @ T[:3, :3].T, T[:3, 3]
    Z = np.min([(d - n @ o) / (dirs @ n) for n, d in PLANES], axis=0)     # inside the room every plane is ahead
    assert (Z > 0).all()
    return prm.f * prm.base / Z


def stereo_pair(pose, shape, prm, seed=0, noise=1.0):
    """(L, R) uint8 images of the scene under a band-limited random texture, as tests/disparity_ref.py's slanted_pair makes them:
    the right pixel xr sees the point whose left column x solves x - d(x, y) = xr (d changes by less than a pixel a column)."""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    d = disparity_exact(pose, shape, prm)
    pad = int(d.max()) + 16
    k = np.exp(-0.5 * (np.arange(-3, 4) / 1.0) ** 2)
    tex = np.stack([np.convolve(rng.normal(size=cols + 2 * pad), k / k.sum(), mode="same") for _ in range(rows)])
    tex = (tex - tex.mean()) / tex.std()
    tex = 0.5 * tex + 0.5 * np.roll(tex, 1, axis=0)
    xs = np.arange(cols, dtype=np.float64)
    left, right = np.zeros(shape), np.zeros(shape)
    for y in range(rows):
        xr_of_x = xs - d[y]
        assert (np.diff(xr_of_x) > 0).all()
        xl = np.interp(xs, xr_of_x, xs, left=np.nan, right=np.nan)
        xl = np.where(np.isnan(xl), xs + d[y, -1], xl)                     # beyond the left view: any texture
        for img, u in ((left, xs), (right, xl)):
            u = u + pad
            i0 = np.floor(u).astype(np.int64)
            img[y] = tex[y, i0] * (1 - (u - i0)) + tex[y, i0 + 1] * (u - i0)
    return tuple(np.clip(np.rint(128 + 40 * im + rng.normal(scale=noise, size=shape)), 0, 255).astype(np.uint8) for im in (left, right))
