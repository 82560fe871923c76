"""Numpy restatement of the maps' eviction (include/viso_hip.h, "Map eviction"): the split of an entry array at a box, the box
around a point, and the table itself: the hash of a key (the finaliser of splitmix64, csrc/voxel_hash.h) and linear probing, with
which the tests build tables whose clusters lie where they want them."""
import numpy as np

BIAS = 1 << 20
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
M64 = (1 << 64) - 1


def keys_of(k):
    k = np.asarray(k).astype(np.int64) + BIAS
    return (k[..., 0] << 42) | (k[..., 1] << 21) | k[..., 2]


def inside(k, lo, hi):
    """bool [n]: lo <= k < hi on every axis, in int64 (the box's entries are any int32)."""
    k = np.asarray(k).astype(np.int64)
    return ((k >= np.asarray(lo, np.int64)) & (k < np.asarray(hi, np.int64))).all(axis=-1)


def split(entries, lo, hi):
    """(kept, evicted) of an entry array of any of the three dtypes, both sorted by key."""
    e = np.asarray(entries)
    e = e[np.argsort(keys_of(e["k"]), kind="stable")]
    m = inside(e["k"], lo, hi)
    return e[m], e[~m]


def box_around(centre, half_side, voxel):
    """(lo, hi) of viso_voxel_box_around: per axis lo = floor((c - r) / voxel), hi = floor((c + r) / voxel) + 1 in double, each
    clamped to int32."""
    lo, hi = [], []
    with np.errstate(over="ignore"):
        quot = [((c - np.float64(half_side)) / np.float64(voxel), (c + np.float64(half_side)) / np.float64(voxel)) for c in np.asarray(centre, np.float64)]
    for a, b in quot:
        a, b = np.floor(a), np.floor(b)
        lo.append(I32_MIN if a <= I32_MIN else I32_MAX if a >= I32_MAX else int(a))
        hi.append(I32_MIN if b + 1 <= I32_MIN else I32_MAX if b >= I32_MAX else int(b) + 1)
    return np.array(lo, np.int32), np.array(hi, np.int32)


def map_hash(key):
    """uint32 of map_hash (csrc/voxel_hash.h) for one key, in Python integers."""
    k = int(key) & M64
    k ^= k >> 30; k = (k * 0xbf58476d1ce4e5b9) & M64
    k ^= k >> 27; k = (k * 0x94d049bb133111eb) & M64
    k ^= k >> 31
    return k & 0xffffffff


def map_hash_np(keys):
    """The same for an array of keys."""
    k = np.asarray(keys).astype(np.uint64)
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(30); k *= np.uint64(0xbf58476d1ce4e5b9)
        k ^= k >> np.uint64(27); k *= np.uint64(0x94d049bb133111eb)
        k ^= k >> np.uint64(31)
    return (k & np.uint64(0xffffffff)).astype(np.int64)


def probe_table(keys, capacity_log2):
    """The table after inserting `keys` (distinct) in their order by linear probing from map_hash(key) & mask: an int64 [slots]
    array of keys, -1 = empty.  More keys than slots is an error."""
    slots = 1 << capacity_log2
    table = np.full(slots, -1, np.int64)
    homes = map_hash_np(keys) & (slots - 1)
    assert len(keys) <= slots
    for key, s in zip(np.asarray(keys, np.int64).tolist(), homes.tolist()):
        while table[s] != -1:
            assert table[s] != key
            s = (s + 1) & (slots - 1)
        table[s] = key
    return table


def clusters(table):
    """[(first slot, length)] of the maximal runs of occupied slots of a table with at least one empty slot, cyclically: a run that
    wraps from the last slot to slot 0 is one cluster, listed with its first slot near the end."""
    occ = table != -1
    n = len(table)
    assert not occ.all()
    out = []
    for s in np.nonzero(occ & ~np.roll(occ, 1))[0].tolist():
        length = 0
        while occ[(s + length) % n]:
            length += 1
        out.append((s, length))
    return out


def reachable(table):
    """True when every key of the table is found by a probe from its home that stops at the first empty slot."""
    n = len(table)
    for slot in np.nonzero(table != -1)[0].tolist():
        s = map_hash(table[slot]) & (n - 1)
        while s != slot:
            if table[s] == -1:
                return False
            s = (s + 1) & (n - 1)
    return True


# ---- hand-made tables: clusters that lie where a test wants them ----------------------------------------------------------------
HAND_LOG2 = 10
HAND_BOX = (np.zeros(3, np.int32), np.full(3, 64, np.int32))   # kept: 0 <= k < 64 on every axis
# (home slot, outside the box) in insertion order.  Inserted one at a time, an entry lies in the first free slot at or after its home,
# so the k-th of a group whose homes do not run ahead of the slots lies k slots after the group's first home.
HAND_WRAP = [(1019, True), (1019, False), (1020, False), (1021, True), (1022, False), (1022, False), (1023, True), (1023, False),
             (1021, False), (1020, True), (0, False), (1, True), (3, False)]                       # slots 1019 .. 1023, 0 .. 7
HAND_LONG = [(300 + i // 3, i in (0, 9, 19)) for i in range(20)]                                   # slots 300 .. 319
HAND_ALONE = [(600, True), (700, False)]                                                           # 599, 601, 699, 701 stay empty


def hand_keys():
    """(k int32 [n][3] in insertion order, outside bool [n]) for HAND_WRAP + HAND_LONG + HAND_ALONE: for each (home, outside) the
    next unused voxel with that home slot, from [0, 64)^3 when it is to stay and from [64, 128) x [0, 64)^2 when it is to leave."""
    g = np.stack(np.meshgrid(*[np.arange(64)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    pools = {}
    for outside in (False, True):
        k = g + np.array([64 if outside else 0, 0, 0])
        homes = map_hash_np(keys_of(k)) & ((1 << HAND_LOG2) - 1)
        pools[outside] = (k, homes)
    used, ks, outs = set(), [], []
    for home, outside in HAND_WRAP + HAND_LONG + HAND_ALONE:
        k, homes = pools[outside]
        i = next(int(i) for i in np.nonzero(homes == home)[0] if (outside, int(i)) not in used)
        used.add((outside, i))
        ks.append(k[i]); outs.append(outside)
    return np.array(ks, np.int32), np.array(outs)


def fill(k, dtype, rng, trunc=3):
    """Entries of `dtype` (any of the three kinds) at the voxels k with random payloads that add_entries accepts."""
    e = np.zeros(len(k), dtype)
    e["k"] = k
    if "count" in dtype.names:
        e["count"] = rng.integers(1, 4, len(k))
        e["sum"] = rng.integers(0, 1024, (len(k), 3)) * e["count"].astype(np.uint64)[:, None]
    else:
        w = rng.integers(1, 4, len(k))
        e["weight"] = w
        e["sum"] = rng.integers(-trunc * 1024, trunc * 1024 + 1, len(k)) * w
        if "gray" in dtype.names:
            e["gray"] = rng.integers(0, 256, len(k)) * w
    return e


TOMB = -2


def evict_table(table, leave):
    """The three passes of the device (csrc/voxel_hash.h) on a table of probe_table with at least one empty slot: the keys in the
    set `leave` become tombstones, every cluster is walked from its first slot and each live key put back at the first tombstone
    at or after its home, the tombstones become empty.  Returns the new table; the input is not changed."""
    t = np.array(table, np.int64)
    n = len(t)
    heads = [s for s, _ in clusters(t)]
    for s in range(n):
        if int(t[s]) in leave:
            t[s] = TOMB
    for head in heads:
        off = 0
        while t[(head + off) % n] != -1:
            s = (head + off) % n
            key = int(t[s])
            if key != TOMB:
                d = (s - (map_hash(key) & (n - 1))) % n
                assert d <= off                      # the home lies in the cluster
                o = off - d
                while o < off and t[(head + o) % n] != TOMB:
                    o += 1
                if o < off:
                    t[(head + o) % n], t[s] = key, TOMB
            off += 1
    t[t == TOMB] = -1
    return t
