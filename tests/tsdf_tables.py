"""Hand-built voxel tables for the TSDF kernels that read a table (tsdf_render_kernel, tsdf_crossings_kernel, tsdf_mesh_kernel in
libviso_amd/csrc/tsdf.hip), shared by tests/test_gpu_mesh.py, tests/test_gpu_render_edges.py and the CPU test of the cases
themselves (tests/test_render_cpu.py).  A fused scene is a large regular structure: neighbouring rays do the same thing at the
same sample, and some branches of the ray casting's rule (tests/render_ref.py) never occur in one.  These tables go to the device
through add_entries.

Every case function returns (entries, voxel, param, shape, pose, max_depth, min_weight): the arguments of render_ref.render.
No device and no library at module level."""
import numpy as np

from libviso_amd import hostmath
from libviso_amd.abi import Param

import render_ref as RR
import tsdf_ref as R

BIAS = R.BIAS
POSE = np.linalg.inv(hostmath.tr2mat([0.013, -0.021, 0.007, 0.31, -0.12, 1.47]))   # the pose of test_gpu_tsdf
TRUNC = 3                                                                          # the maps' default trunc_voxels
BIG = 1 << 31                                                                      # a weight beyond int32


def random_block(rng, n=9, origin=-4, occupancy=0.7, trunc=TRUNC):
    """n^3 voxels from `origin` (one number or one per axis), each present with probability `occupancy`; weights 1..3; sums over
    the whole band with an eighth each at 0 and at both ends of it, and some that are no multiple of the weight.  Sorted by key."""
    g = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) + np.asarray(origin, np.int64)
    g = g[rng.random(len(g)) < occupancy]
    e = np.zeros(len(g), R.ENTRY)
    e["k"] = g
    e["weight"] = rng.integers(1, 4, len(g))
    lim = trunc * 1024
    q = rng.integers(-lim, lim + 1, len(g))
    special = rng.integers(0, 8, len(g))
    q = np.where(special == 0, 0, np.where(special == 1, lim, np.where(special == 2, -lim, q)))
    e["sum"] = q * e["weight"].astype(np.int64)
    # sums that are no multiple of the weight: the mean is not an integer
    odd = (e["weight"] > 1) & (np.abs(e["sum"]) < lim) & (special > 4)
    e["sum"][odd] += 1
    return e[np.argsort(R.keys_of(e["k"]))]


def _layer(kz, half, weight, total):
    g = np.stack(np.meshgrid(np.arange(-half, half), np.arange(-half, half), indexing="ij"), axis=-1).reshape(-1, 2)
    e = np.zeros(len(g), R.ENTRY)
    e["k"][:, :2], e["k"][:, 2] = g, kz
    e["weight"], e["sum"] = weight, total
    return e


def slab(kz, half=8, weight=2, sum_pos=None, sum_neg=None):
    """A surface seen from -z: the layer of voxels at kz with the sum sum_pos >= 0 (default 300 weight) and the one at kz + 1 with
    sum_neg < 0 (default -500 weight), each over [-half, half)^2 in kx, ky.  Sorted by key."""
    sum_pos = 300 * weight if sum_pos is None else sum_pos
    sum_neg = -500 * weight if sum_neg is None else sum_neg
    assert sum_pos >= 0 > sum_neg
    return R.merge(_layer(kz, half, weight, sum_pos), _layer(kz + 1, half, weight, sum_neg))


def param(f=721.5377, cu=4.3, cv=2.6, base=0.5371):
    return Param.default(base=base, f=f, cu=cu, cv=cv)


def events(case):
    """(disparity, weight, Counter of render_ref.EVENTS) of a case by the loop restatement."""
    from collections import Counter
    trace = Counter()
    d, w = RR.render_loop(*case, trace=trace)
    return d, w, trace


# ---- random blocks: every lane of a wave at a different place in the rule -----------------------------------------------------
BLOCK_POSES = {"none": None, "sideways": RR.sideways(None, 0.15, 0.05), "rigid": POSE}
BLOCK_MIN_WEIGHTS = (1, 2, 3)
# seed, n, origin, occupancy, (f, cu, cv), shape, max_depth (N = 40 and 30 samples), the poses of the sweep
BLOCKS = {"far": (3, 12, (-6, -6, 1), 0.7, (100.0, 99.5, 11.5), (24, 200), 4.0, ("none", "sideways", "rigid")),
          "inside": (3, 10, (-5, -5, 0), 0.6, (60.0, 64.5, 9.5), (20, 130), 3.0, ("none",))}    # the camera in the block's first layer
BLOCK_EVENTS = ("backface", "negative_after_unusable", "negative_after_negative", "front_sum_zero", "zero_after_positive",
                "underweight", "first_negative")


def block_entries(name):
    seed, n, origin, occupancy = BLOCKS[name][:4]
    return random_block(np.random.default_rng(seed), n=n, origin=origin, occupancy=occupancy)


def block_view(name, pose="none", min_weight=1, entries=None):
    (f, cu, cv), shape, max_depth = BLOCKS[name][4:7]
    return (block_entries(name) if entries is None else entries, 0.2, param(f, cu, cv), shape, BLOCK_POSES[pose], max_depth, min_weight)


def block_sweep(name):
    """[(pose name, min_weight, case)] over the poses of the block and min_weight 1, 2, 3, all of one table."""
    e = block_entries(name)
    return [(p, mw, block_view(name, p, mw, e)) for p in BLOCKS[name][7] for mw in BLOCK_MIN_WEIGHTS]


def chains_view(min_weight=1):
    """A 9^3 block at 96 % occupancy, at most 729 voxels: in a table of 2^10 slots the march's lookups walk chains of tens of slots
    that wrap the table's end.  Off the axis and a metre away, so that the rays at the left miss it."""
    e = random_block(np.random.default_rng(10), n=9, origin=(-2, -4, 5), occupancy=0.96)
    return (e, 0.2, param(100.0, 99.5, 11.5), (24, 200), None, 4.0, min_weight)


# ---- a hit whose value is invalid ends the march -------------------------------------------------------------------------------
SMALL = (5, 9)


def too_big():
    """A surface 0.09 m before the camera (v = 66140 >= 32768) and a valid one at 2.04 m behind it: every pixel INVALID."""
    return (R.merge(slab(1), slab(40)), 0.05, param(), SMALL, None, 4.0, 1)


def too_big_alone():
    """The far surface of too_big alone: 3034 at every pixel."""
    return (slab(40), 0.05, param(), SMALL, None, 4.0, 1)


def too_small():
    """f base so small that the surface at 8.2 m has v = 0.7 < 1: every pixel INVALID."""
    return (slab(40, half=40), 0.2, param(f=10.0, base=0.01), SMALL, None, 20.0, 1)


def behind():
    """The camera at the centre of voxel (0, 0, 0) of a block around it, under the rotation of POSE.  That voxel has sum 0 and its
    centre the depth 0 exactly (512 s = 0.1), so a hit in front of which it lies has t = 0 and zs = 0: !(zs > 0), INVALID."""
    e = random_block(np.random.default_rng(5), n=10, origin=(-5, -5, -5), occupancy=0.9)
    T = POSE.copy()
    T[:3, 3] = 0.1
    return (e, 0.2, param(60.0, 64.5, 9.5), (20, 130), T, 1.0, 1)


# ---- gaps: samples outside the key range ---------------------------------------------------------------------------------------
GAP_VOXEL = 0.05
EDGE = float(R.RANGE) * GAP_VOXEL / 1024.0      # the key range is [-EDGE, EDGE) on every axis: 52428.8 m


def _at(x, y, z):
    T = np.eye(4)
    T[:3, 3] = x, y, z
    return T


def gap_in():
    """From 0.3 m below the range's first voxels along z: the first samples of every ray are gaps, then a slab (7349)."""
    return (slab(-BIAS + 10), GAP_VOXEL, param(), SMALL, _at(0.0, 0.0, -EDGE - 0.3), 3.0, 1)


def gap_out():
    """From 1 m inside the range's end along z: the slab (13973) is so narrow that the rays to both sides of it pass it, run out
    of the range and end in gaps."""
    return (slab(BIAS - 12, half=2), GAP_VOXEL, param(cu=249.3, cv=1.2), (3, 500), _at(0.0, 0.0, EDGE - 1.0), 3.0, 1)


def gap_beside():
    """Beside the last voxels of all three axes: the slab of gap_out is 52 km away, every ray leaves the range and sees nothing."""
    return (slab(BIAS - 12, half=2), GAP_VOXEL, param(), SMALL, _at(EDGE - 0.3, EDGE - 0.3, EDGE - 1.0), 3.0, 1)


# ---- weights and means ---------------------------------------------------------------------------------------------------------
def weights_and_means():
    """A slab at kz = 10 of voxel 0.2 whose columns kx come in bands, front layer (wa, sa) and back layer (wb, sb):
      kx in -8 .. -7   both sums at the ends of the band, +-T 1024 w, with wa = 3 > wb = 1
      kx in -6 .. -1   wa = 3 > wb = 2, sums that are no multiple of the weight
      kx in  0 ..  3   wa = 2 < wb = 5, likewise
      kx in  4 ..  5   wa = wb = 2^31
      kx in  6 ..  7   wa = 2^31 > wb = 3
    The view spans all of them and a few columns beside the slab."""
    kz, half, lim = 10, 8, TRUNC * 1024
    front, back = _layer(kz, half, 1, 0), _layer(kz + 1, half, 1, 0)
    kx = front["k"][:, 0]
    assert np.array_equal(kx, back["k"][:, 0])
    bands = [(kx < -6, 3, 1, lim * 3, -lim * 1), ((kx >= -6) & (kx < 0), 3, 2, 301 * 3 + 1, -500 * 2 - 1),
             ((kx >= 0) & (kx < 4), 2, 5, 299 * 2 + 1, -501 * 5 + 2), ((kx >= 4) & (kx < 6), BIG, BIG, 700 * BIG + 1, -200 * BIG - 1),
             (kx >= 6, BIG, 3, 100 * BIG + 3, -900 * 3 + 1)]
    for sel, wa, wb, sa, sb in bands:
        front["weight"][sel], front["sum"][sel], back["weight"][sel], back["sum"][sel] = wa, sa, wb, sb
    return (R.merge(front, back), 0.2, param(100.0, 79.5, 2.5), (6, 160), None, 4.0, 1)


# name: (case function, the event the case exists for)
SMALL_CASES = {"too_big": (too_big, "hit_too_big"), "too_big_alone": (too_big_alone, "hit"), "too_small": (too_small, "hit_too_small"),
               "behind": (behind, "hit_behind"),               "gap_in": (gap_in, "gap"), "gap_out": (gap_out, "gap"), "gap_beside": (gap_beside, "gap"),
               "weights_and_means": (weights_and_means, "hit")}


# ---- the tables of the crossings -----------------------------------------------------------------------------------------------
CROSSING_PLACES = {"origin": -4, "top": BIAS - 9, "bottom": -BIAS}


def crossing_block(place):
    """The 9^3 block of test_gpu_mesh.test_random_block.  top: its last voxels are the last of every axis, which have no neighbour
    there; bottom: its first are the first."""
    return random_block(np.random.default_rng(9), origin=CROSSING_PLACES[place])


def chains_block():
    """The block of test_gpu_mesh.test_long_probe_chains: about 700 voxels for a table of 2^10 slots."""
    return random_block(np.random.default_rng(10), occupancy=0.96)
