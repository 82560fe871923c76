"""The handles and the two-pass getters of the voxel map and the TSDF map through raw ctypes (include/viso_hip.h, viso_map_* /
viso_tsdf_*; the shared table layer, libviso_amd/csrc/voxel_host.h): what both kinds promise alike and no wrapper may paper over.
A short list, an exact one, an empty table, a threshold of 0, destroy, and a handle of one kind given to the other kind."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import (MAP_ENTRY_DTYPE, TSDF_CROSSING_DTYPE, TSDF_ENTRY_DTYPE, MapCounters, MapParams, TsdfCounters,
                             TsdfParams)

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 1, -1
SENTINEL = 0xA5
# a dozen voxels: six pairs of neighbours along x, y, z, x, y, z, far from each other, on both sides of the origin
PAIRS = [((-40 + 15 * i, 7 - 5 * i, -3 + 11 * i), i % 3) for i in range(6)]


def _voxels():
    out = []
    for k, axis in PAIRS:
        nb = list(k)
        nb[axis] += 1
        out += [k, tuple(nb)]
    return out


def _map_entries():
    e = np.zeros(12, MAP_ENTRY_DTYPE)
    for i, k in enumerate(_voxels()):
        e[i] = (k, 2 + i, (5 * i, 1023 * (2 + i), 17))
    return e


def _tsdf_entries():
    e = np.zeros(12, TSDF_ENTRY_DTYPE)
    for i, k in enumerate(_voxels()):
        e[i] = (k, 1 + i, (100 + 7 * i) * (1 if i % 2 == 0 else -1))   # the two voxels of a pair: opposite signs
    return e


def _by_key(a, extra=()):
    cols = [a[f] for f in reversed(extra)] + [a["k"][:, 2], a["k"][:, 1], a["k"][:, 0]]
    return a[np.lexsort(cols)]


def _want_crossings():
    e = _tsdf_entries()
    c = np.zeros(6, TSDF_CROSSING_DTYPE)
    for i, (k, axis) in enumerate(PAIRS):
        a, b = e[2 * i], e[2 * i + 1]
        c[i] = (k, axis, a["weight"], b["weight"], a["sum"], b["sum"])
    return _by_key(c, ("axis",))


# kind, the count and get functions, the list's dtype, the list the dozen entries give
GETTERS = [
    ("map", "viso_map_count", "viso_map_get", MAP_ENTRY_DTYPE, lambda: _by_key(_map_entries())),
    ("tsdf", "viso_tsdf_count", "viso_tsdf_get", TSDF_ENTRY_DTYPE, lambda: _by_key(_tsdf_entries())),
    ("tsdf", "viso_tsdf_surface_count", "viso_tsdf_surface", TSDF_CROSSING_DTYPE, _want_crossings),
]


def _create(L, kind):
    h = C.c_void_p()
    if kind == "map":
        p = MapParams(voxel=0.2, min_disp16=16, capacity_log2=10)
        assert L.viso_map_create(None, C.byref(p), C.byref(h)) == OK
    else:
        p = TsdfParams(voxel=0.2, trunc_voxels=3, min_disp16=16, capacity_log2=10)
        assert L.viso_tsdf_create(None, C.byref(p), C.byref(h)) == OK
    assert h.value
    return h


def _fill(L, kind, h):
    e = _map_entries() if kind == "map" else _tsdf_entries()
    assert getattr(L, f"viso_{kind}_add_entries")(h, e.ctypes.data, len(e)) == OK


@pytest.mark.parametrize("kind,count_name,get_name,dtype,want", GETTERS, ids=[g[2] for g in GETTERS])
def test_getter_pair(kind, count_name, get_name, dtype, want):
    L = libviso_amd.load()
    count, get, destroy = getattr(L, count_name), getattr(L, get_name), getattr(L, f"viso_{kind}_destroy")
    want = want()
    h = _create(L, kind)
    try:
        n = C.c_size_t(99)
        # an empty table: a null list of no room is fine
        assert get(h, 1, None, 0, C.byref(n)) == OK and n.value == 0
        _fill(L, kind, h)
        assert count(h, 1, C.byref(n)) == OK and n.value == len(want)
        # a threshold of 0 is no threshold
        assert count(h, 0, C.byref(n)) == ERR_ARG
        buf = np.full(len(want) * dtype.itemsize, SENTINEL, np.uint8)
        assert get(h, 0, buf.ctypes.data, len(want), C.byref(n)) == ERR_ARG
        # one short: the true count comes back, the list is not touched
        n.value = 99
        assert get(h, 1, buf.ctypes.data, len(want) - 1, C.byref(n)) == ERR_ARG
        assert n.value == len(want) and np.all(buf == SENTINEL)
        # exact: sorted by the documented key
        n.value = 99
        assert get(h, 1, buf.ctypes.data, len(want), C.byref(n)) == OK and n.value == len(want)
        got = buf.view(dtype)
        assert got.tobytes() == want.tobytes(), (got, want)
    finally:
        assert destroy(h) == OK
    assert destroy(h) == ERR_ARG      # no longer a live handle: refused without being looked into
    assert destroy(None) == OK


def test_handle_of_the_other_kind():
    L = libviso_amd.load()
    m, t = _create(L, "map"), _create(L, "tsdf")
    try:
        _fill(L, "map", m)
        _fill(L, "tsdf", t)
        mc, tc = MapCounters(), TsdfCounters()
        assert L.viso_map_stats(t, C.byref(mc)) == ERR_ARG and L.viso_map_clear(t) == ERR_ARG
        assert L.viso_tsdf_stats(m, C.byref(tc)) == ERR_ARG and L.viso_tsdf_clear(m) == ERR_ARG
        # neither was cleared or otherwise touched, and both go on working
        n = C.c_size_t()
        assert L.viso_map_count(m, 1, C.byref(n)) == OK and n.value == 12
        assert L.viso_tsdf_count(t, 1, C.byref(n)) == OK and n.value == 12
        assert L.viso_map_stats(m, C.byref(mc)) == OK and mc.n_occupied == 12 and mc.n_dropped == 0
        assert L.viso_tsdf_stats(t, C.byref(tc)) == OK and tc.n_occupied == 12 and tc.n_dropped == 0
        assert L.viso_map_clear(m) == OK and L.viso_map_count(m, 1, C.byref(n)) == OK and n.value == 0
        assert L.viso_tsdf_clear(t) == OK and L.viso_tsdf_count(t, 1, C.byref(n)) == OK and n.value == 0
    finally:
        assert L.viso_map_destroy(m) == OK and L.viso_tsdf_destroy(t) == OK
