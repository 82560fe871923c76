"""The three per-slot kernels that every kind of voxel table shares (libviso_amd/csrc/voxel_hash.h: add_entries, the getters'
compaction, clear), through the public calls of all three kinds of map at the smallest table, capacity_log2 = 10.  Every expected
value is an exact integer from a dictionary on the host: no tolerances.  The exactly full table, the overflow and its recovery are
tests/test_gpu_evict.py's."""
import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import MAP_ENTRY_DTYPE, TSDF_ENTRY_DTYPE, TSDF_GRAY_ENTRY_DTYPE

pytestmark = pytest.mark.gpu

KINDS = ("map", "tsdf", "gray")
DTYPE = dict(map=MAP_ENTRY_DTYPE, tsdf=TSDF_ENTRY_DTYPE, gray=TSDF_GRAY_ENTRY_DTYPE)
TRUNC = 3
LIM = 1024 * TRUNC                       # |sum| <= LIM weight
LO, HI = -(1 << 20), (1 << 20) - 1       # the corners of the key range
UNIT = dict(map="count", tsdf="weight", gray="weight")


def _make(kind):
    if kind == "map":
        return libviso_amd.VoxelMap(None, voxel=0.2, capacity_log2=10)
    return libviso_amd.TsdfMap(None, gray=kind == "gray", voxel=0.2, trunc_voxels=TRUNC, capacity_log2=10)


def _entries(kind, m, threshold=1):
    return m.entries(threshold, gray=True) if kind == "gray" else m.entries(threshold)


def _entry(kind, k, units, top=0):
    """One entry at voxel k.  top: 0 the smallest payload of `units`, +1 / -1 the largest legal one (a TSDF sum of that sign)."""
    e = np.zeros(1, DTYPE[kind])
    e["k"], e[UNIT[kind]] = k, units
    if kind == "map":
        e["sum"] = 1023 * units if top else 0
    else:
        e["sum"] = top * LIM * units
        if kind == "gray":
            e["gray"] = 255 * units if top else 0
    return e


def _random(kind, rng, n):
    """n entries: distinct random keys, a quarter of the entries on keys that are already there; the corners of the key range; of
    every four entries one with the largest legal payload."""
    n_keys = max(1, n - n // 4)
    keys = set()
    for corner in ((LO, LO, LO), (HI, HI, HI), (LO, HI, 0))[:n_keys]:
        keys.add(corner)
    while len(keys) < n_keys:
        keys.add(tuple(int(v) for v in rng.integers(LO, HI + 1, 3)))
    keys = sorted(keys)
    keys += [keys[int(i)] for i in rng.integers(0, n_keys, n - n_keys)]
    out = np.zeros(n, DTYPE[kind])
    for i, k in enumerate(keys):
        units = int(rng.integers(1, 1000))
        if i % 4 == 0:
            out[i] = _entry(kind, k, units, top=1 if i % 8 == 0 else -1)[0]
            continue
        out[i] = _entry(kind, k, units)[0]
        if kind == "map":
            out["sum"][i] = rng.integers(0, 1023 * units + 1, 3)
        else:
            out["sum"][i] = int(rng.integers(-LIM * units, LIM * units + 1))
            if kind == "gray":
                out["gray"][i] = int(rng.integers(0, 255 * units + 1))
    return out[rng.permutation(n)]


def _key(k):
    return ((int(k[0]) - LO) << 42) | ((int(k[1]) - LO) << 21) | (int(k[2]) - LO)


def _merged(kind, entries, threshold=1):
    """The table after `entries`, from a dictionary: the getter's array of the voxels at or above the threshold, sorted by key."""
    fields = [f for f in DTYPE[kind].names if f != "k"]
    table = {}
    for e in entries:
        slot = table.setdefault(_key(e["k"]), dict(k=tuple(int(v) for v in e["k"]), **{f: 0 for f in fields}))
        for f in fields:
            slot[f] = slot[f] + (e[f].astype(object) if e[f].ndim else int(e[f]))
    rows = [table[key] for key in sorted(table) if table[key][UNIT[kind]] >= threshold]
    out = np.zeros(len(rows), DTYPE[kind])
    for i, row in enumerate(rows):
        for f, v in row.items():
            out[i][f] = v
    return out


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _stats(kind, entries):
    """The statistics of a cleared table after add_entries(entries)."""
    units = sum(int(u) for u in entries[UNIT[kind]])
    occupied = len({_key(k) for k in entries["k"]})
    if kind == "map":
        return dict(n_points=units, n_inserts=len(entries), n_out_of_range=0, n_dropped=0, n_occupied=occupied)
    return dict(n_points=0, n_updates=units, n_out_of_range=0, n_dropped=0, n_occupied=occupied)


@pytest.mark.parametrize("n", (1, 64, 65, 257))   # one lane, a full wave, a wave and a lane, a second workgroup of one lane
@pytest.mark.parametrize("kind", KINDS)
def test_add_entries_sizes(kind, n):
    e = _random(kind, np.random.default_rng(100 + n), n)
    want = _merged(kind, e)
    assert n == 1 or len(want) < n                # keys repeat within the call: their atomics add
    m = _make(kind)
    m.add_entries(e)
    got = _entries(kind, m)
    assert _same(got, want), (got, want)
    assert m._count("count", 1).value == len(want)
    assert m.stats() == _stats(kind, e)
    m.close()


@pytest.mark.parametrize("kind", KINDS)
def test_add_entries_twice_and_key_corners(kind):
    """Two calls add up like one; the voxels at the corners of the key range, with the largest legal payloads of either sign."""
    a = np.concatenate([_entry(kind, (LO, LO, LO), 7, top=1), _entry(kind, (HI, HI, HI), 9, top=-1), _entry(kind, (LO, HI, LO), 1)])
    b = np.concatenate([_entry(kind, (HI, HI, HI), 2, top=-1), _entry(kind, (HI, LO, HI), 1000, top=1)])
    m = _make(kind)
    m.add_entries(a)
    m.add_entries(b)
    both = np.concatenate([a, b])
    want = _merged(kind, both)
    assert len(want) == 4 and [tuple(k) for k in want["k"]] == [(LO, LO, LO), (LO, HI, LO), (HI, LO, HI), (HI, HI, HI)]
    assert _same(_entries(kind, m), want)
    st = _stats(kind, both)
    assert m.stats() == st and st["n_occupied"] == 4
    m.close()


@pytest.mark.parametrize("kind", KINDS)
def test_threshold(kind):
    """Counts / weights 1, 2 and 3 (the 3s added up from 1 + 2 in one call): the getters at min = 1 .. 4."""
    rng = np.random.default_rng(7)
    keys = [tuple(int(v) for v in rng.integers(-50, 50, 3)) + (i,) for i in range(9)]
    keys = [(k[0], k[1], k[3]) for k in keys]     # distinct along z
    parts = [_entry(kind, k, 1, top=1) for k in keys[:3]] + [_entry(kind, k, 2) for k in keys[3:5]]
    for k in keys[5:]:
        parts += [_entry(kind, k, 1), _entry(kind, k, 2, top=-1)]
    e = np.concatenate(parts)
    m = _make(kind)
    m.add_entries(e)
    for threshold, n in ((1, 9), (2, 6), (3, 4), (4, 0)):
        want = _merged(kind, e, threshold)
        assert len(want) == n
        assert m._count("count", threshold).value == n
        assert _same(_entries(kind, m, threshold), want)
    m.close()


@pytest.mark.parametrize("kind", KINDS)
def test_clear_leaves_nothing(kind):
    e = _random(kind, np.random.default_rng(3), 257)
    m = _make(kind)
    m.add_entries(e)
    assert len(_entries(kind, m)) > 150
    m.clear()
    assert len(_entries(kind, m)) == 0 and m._count("count", 1).value == 0
    assert m.stats() == _stats(kind, e[:0]) and set(m.stats().values()) == {0}
    # the smallest entry at a voxel that held the largest payloads: nothing of them is left, the gray word included
    units = e[UNIT[kind]].astype(np.int64)
    is_top = (e["sum"][:, 0] == 1023 * units) if kind == "map" else (e["sum"] == LIM * units) & (e["gray" if kind == "gray" else "sum"] != 0)
    assert is_top.sum() >= 30
    top = e[is_top][0]
    one = _entry(kind, tuple(int(v) for v in top["k"]), 1)
    m.add_entries(one)
    assert _same(_entries(kind, m), one)
    assert m.stats() == _stats(kind, one)
    # and at every voxel the table held
    m.clear()
    ones = np.concatenate([_entry(kind, tuple(int(v) for v in k), 1) for k in _merged(kind, e)["k"]])
    m.add_entries(ones)
    assert _same(_entries(kind, m), _merged(kind, ones))
    m.close()
