"""Every entry point of the map layer that takes a handle (voxelmap.hip, tsdf.hip, tsdf_align.hip, tsdf_field.hip, tsdf_travel.hip;
create and destroy left out), with arguments that are otherwise valid, against the five states a handle can be in: destroyed, a live
handle of the other kind, a map whose context was destroyed, an overflowed map, a healthy map.  viso_last_error() is compared whole,
a refused call must leave its outputs as they were (zero), and the handle's stats must answer afterwards as they did before.  Every
expected text is read from the C sources (voxel_host.hip: voxel_enter, voxel_refuse_overflowed; the registries' words in
voxelmap.hip and tsdf.hip), never from a run.  What the sources say beside the table of the states: viso_tsdf_is_gray asks the
registry only, so it also answers for a map without a context; clear, stats, is_gray and the two fuse-option calls do not refuse an
overflowed map."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd.abi import (MAP_ENTRY_DTYPE, TSDF_ALIGNMENT_DTYPE, TSDF_ALIGNMENT_GRAY_DTYPE, TSDF_CROSSING_DTYPE, TSDF_ENTRY_DTYPE,
                             TSDF_GRAY_ENTRY_DTYPE, TSDF_MESH_VERTEX_DTYPE, TSDF_NORMAL_DTYPE, TSDF_NORMAL_GRAY_DTYPE, MapCounters, Param,
                             TsdfCounters, VoxelBox)

pytestmark = pytest.mark.gpu

OK, ARG, NOMEM = 1, -1, -4   # VISO_OK, VISO_ERR_ARG, VISO_ERR_NOMEM (include/viso_hip.h)
# the words of the two kinds (VoxelKind): handle, noun, unit, clear_fn
WORDS = {"map": ("map", "map", "points", "viso_map_clear"), "tsdf": ("TSDF", "TSDF map", "updates", "viso_tsdf_clear")}
NOT_REFUSING = ("clear", "stats", "is_gray", "set_fuse_options", "get_fuse_options")   # an overflowed map answers these

# the arguments: one 4 x 8 map and image, one entry, one vertex, a box of 2 x 2 x 2 voxels, one goal, one view
M, IMG = np.full((4, 8), 16, np.int16), np.full((4, 8), 7, np.uint8)
PRM = Param.default(base=1.0, f=2.0, cu=0.0, cv=0.0)
BOX = VoxelBox((C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(2, 2, 2))
GOAL = np.zeros((1, 3), np.int32)
CAP = 1024   # no list of a table of 2^10 slots is longer (a mesh's: below)


def _one(dtype, **fields):
    a = np.zeros(1, dtype)
    for k, v in fields.items():
        a[k] = v
    return a


MAP_ENTRY, TSDF_ENTRY = _one(MAP_ENTRY_DTYPE, count=1), _one(TSDF_ENTRY_DTYPE, weight=1)
GRAY_ENTRY, VERTEX = _one(TSDF_GRAY_ENTRY_DTYPE, weight=1, gray=7), _one(TSDF_MESH_VERTEX_DTYPE, dir=1)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _calls(L):
    """(family, name, kind, make) of every entry point; kind: the TSDF map the call is for ("plain", "gray", "either"; a voxel map's
    are "either"); make(h) gives the call on the handle h and the outputs it may write, all zero."""
    P, z, sz = C.byref, np.zeros, C.c_size_t
    ap, agp = libviso_amd.tsdf_align_params(), libviso_amd.tsdf_align_gray_params()
    mi, ii = _p(M, C.c_int16), _p(IMG, C.c_uint8)
    T = []

    def add(family, name, kind, make):
        T.append((family, name, kind, make))

    def lister(fn, dtype, *front):   # fn(h, *front, out, cap, &n)
        def make(h):
            out, n = z(CAP, dtype), sz()
            return (lambda: fn(h, *front, out.ctypes.data, CAP, P(n))), [out, n]
        return make

    def counter(fn, *front):   # fn(h, *front, &n)
        def make(h):
            n = sz()
            return (lambda: fn(h, *front, P(n))), [n]
        return make

    def stats(fn, counters):
        def make(h):
            c = counters()
            return (lambda: fn(h, P(c))), [c]
        return make

    def render(fn, third):   # third: None, or the dtype and the values a pixel of the third output
        def make(h):
            d, w = z((4, 8), np.int16), z((4, 8), np.uint32)
            extra = [z((4, 8) + third[2:], third[0])] if third else []
            return (lambda: fn(h, 1, P(PRM), 4, 8, 4.0, None, 1, _p(d, C.c_int16), _p(w, C.c_uint32), *[_p(e, third[1]) for e in extra])), [d, w] + extra
        return make

    def linearize(fn, params, dtype, *image):
        def make(h):
            out = z(1, dtype)
            return (lambda: fn(h, P(params), mi, *image, 4, 8, P(PRM), None, out.ctypes.data)), [out]
        return make

    def align(fn, params, dtype, *image):
        def make(h):
            rec = z(1, dtype)
            return (lambda: fn(h, P(params), mi, *image, 4, 8, P(PRM), None, rec.ctypes.data, None, 0)), [rec]
        return make

    add("map", "clear", "either", lambda h: ((lambda: L.viso_map_clear(h)), []))
    add("map", "fuse", "either", lambda h: ((lambda: L.viso_map_fuse(h, mi, 4, 8, P(PRM), None)), []))
    add("map", "add_entries", "either", lambda h: ((lambda: L.viso_map_add_entries(h, MAP_ENTRY.ctypes.data, 1)), []))
    add("map", "count", "either", counter(L.viso_map_count, 1))
    add("map", "get", "either", lister(L.viso_map_get, MAP_ENTRY_DTYPE, 1))
    add("map", "evict_count", "either", counter(L.viso_map_evict_count, P(BOX)))
    add("map", "evict", "either", lister(L.viso_map_evict, MAP_ENTRY_DTYPE, P(BOX)))
    add("map", "stats", "either", stats(L.viso_map_stats, MapCounters))

    add("tsdf", "set_fuse_options", "either", lambda h: ((lambda: L.viso_tsdf_set_fuse_options(h, 0, -1, 255, 0.0)), []))

    def get_options(h):
        c, s, m, n = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_double()
        return (lambda: L.viso_tsdf_get_fuse_options(h, P(c), P(s), P(m), P(n))), [c, s, m, n]
    add("tsdf", "get_fuse_options", "either", get_options)

    def is_gray(h):
        out = C.c_int()
        return (lambda: L.viso_tsdf_is_gray(h, P(out))), [out]
    add("tsdf", "is_gray", "either", is_gray)
    add("tsdf", "clear", "either", lambda h: ((lambda: L.viso_tsdf_clear(h)), []))
    add("tsdf", "fuse", "plain", lambda h: ((lambda: L.viso_tsdf_fuse(h, mi, 4, 8, P(PRM), None)), []))
    add("tsdf", "fuse_gray", "gray", lambda h: ((lambda: L.viso_tsdf_fuse_gray(h, mi, ii, 4, 8, P(PRM), None)), []))
    add("tsdf", "add_entries", "plain", lambda h: ((lambda: L.viso_tsdf_add_entries(h, TSDF_ENTRY.ctypes.data, 1)), []))
    add("tsdf", "add_gray_entries", "gray", lambda h: ((lambda: L.viso_tsdf_add_gray_entries(h, GRAY_ENTRY.ctypes.data, 1)), []))
    add("tsdf", "count", "either", counter(L.viso_tsdf_count, 1))
    add("tsdf", "get", "either", lister(L.viso_tsdf_get, TSDF_ENTRY_DTYPE, 1))
    add("tsdf", "get_gray", "gray", lister(L.viso_tsdf_get_gray, TSDF_GRAY_ENTRY_DTYPE, 1))
    add("tsdf", "evict_count", "either", counter(L.viso_tsdf_evict_count, P(BOX)))
    add("tsdf", "evict", "plain", lister(L.viso_tsdf_evict, TSDF_ENTRY_DTYPE, P(BOX)))
    add("tsdf", "evict_gray", "gray", lister(L.viso_tsdf_evict_gray, TSDF_GRAY_ENTRY_DTYPE, P(BOX)))
    add("tsdf", "surface_count", "either", counter(L.viso_tsdf_surface_count, 1))

    def surface(h):   # a voxel has three crossings at the most
        out, n = z(3 * CAP, TSDF_CROSSING_DTYPE), sz()
        return (lambda: L.viso_tsdf_surface(h, 1, out.ctypes.data, len(out), P(n))), [out, n]
    add("tsdf", "surface", "either", surface)

    def mesh_count(h):
        nv, nt = sz(), sz()
        return (lambda: L.viso_tsdf_mesh_count(h, 1, P(nv), P(nt))), [nv, nt]
    add("tsdf", "mesh_count", "either", mesh_count)

    def mesh(h):   # a voxel has seven edges and its cell six tetrahedra of at most two triangles each
        v, tri, nv, nt = z(7 * CAP, TSDF_MESH_VERTEX_DTYPE), z((12 * CAP, 3), np.uint32), sz(), sz()
        return (lambda: L.viso_tsdf_mesh(h, 1, v.ctypes.data, len(v), tri.ctypes.data, len(tri), P(nv), P(nt))), [v, tri, nv, nt]
    add("tsdf", "mesh", "either", mesh)
    add("tsdf", "render", "either", render(L.viso_tsdf_render, None))
    add("tsdf", "render_gray", "gray", render(L.viso_tsdf_render_gray, (np.uint8, C.c_uint8)))
    add("tsdf", "render_normals", "either", render(L.viso_tsdf_render_normals, (np.float32, C.c_float, 3)))

    def vertex_gray(h):
        g, n = z(1, np.uint8), sz()
        return (lambda: L.viso_tsdf_vertex_gray(h, VERTEX.ctypes.data, 1, _p(g, C.c_uint8), P(n))), [g, n]
    add("tsdf", "vertex_gray", "gray", vertex_gray)

    def vertex_normals(h):
        nrm, n = z((1, 3), np.float32), sz()
        return (lambda: L.viso_tsdf_vertex_normals(h, 1, VERTEX.ctypes.data, 1, _p(nrm, C.c_float), P(n))), [nrm, n]
    add("tsdf", "vertex_normals", "either", vertex_normals)
    add("tsdf", "stats", "either", stats(L.viso_tsdf_stats, TsdfCounters))
    add("tsdf", "linearize", "either", linearize(L.viso_tsdf_linearize, ap, TSDF_NORMAL_DTYPE))
    add("tsdf", "align", "either", align(L.viso_tsdf_align, ap, TSDF_ALIGNMENT_DTYPE))
    add("tsdf", "linearize_gray", "gray", linearize(L.viso_tsdf_linearize_gray, agp, TSDF_NORMAL_GRAY_DTYPE, ii))
    add("tsdf", "align_gray", "gray", align(L.viso_tsdf_align_gray, agp, TSDF_ALIGNMENT_GRAY_DTYPE, ii))

    def distance_field(h):
        sq, st, n = z(8, np.uint32), z(8, np.uint8), sz()
        return (lambda: L.viso_tsdf_distance_field(h, 1, P(BOX), 0, _p(sq, C.c_uint32), _p(st, C.c_uint8), 8, P(n))), [sq, st, n]
    add("tsdf", "distance_field", "either", distance_field)

    def travel_field(h):
        cost, sq, st, used, reached, rounds = z(8, np.uint32), z(8, np.uint32), z(8, np.uint8), sz(), sz(), sz()
        return (lambda: L.viso_tsdf_travel_field(h, 1, P(BOX), 0, 0, _p(GOAL, C.c_int32), 1, _p(cost, C.c_uint32), _p(sq, C.c_uint32),
                                                 _p(st, C.c_uint8), 8, P(used), P(reached), P(rounds))), [cost, sq, st, used, reached, rounds]
    add("tsdf", "travel_field", "either", travel_field)
    assert len(T) == 38 and len({(f, n) for f, n, _, _ in T}) == 38
    return T


def _maps(ctx):
    """One map of each kind on ctx, with the parameters of an overflowed one: {"map", "plain", "gray"}."""
    kw = dict(voxel=0.5, min_disp16=1, capacity_log2=10)
    return {"map": libviso_amd.VoxelMap(ctx, **kw), "plain": libviso_amd.TsdfMap(ctx, trunc_voxels=1, **kw),
            "gray": libviso_amd.TsdfMap(ctx, gray=True, trunc_voxels=1, **kw)}


def _overflow(maps):
    """The existing 1 x 2000 map, which none of the tables of 1024 slots holds."""
    wide, img = np.full((1, 2000), 16, np.int16), np.full((1, 2000), 7, np.uint8)
    for which, t in maps.items():
        with pytest.raises(libviso_amd.VisoError, match="-4"):
            t.fuse(wide, PRM, **(dict(image=img) if which == "gray" else {}))


def _handles(kind, hs):
    """The handles of `hs` that a call of this kind goes to."""
    return [hs["plain"], hs["gray"]] if kind == "either" else [hs[kind]]


def _stats(L, family, h):
    """viso_*_stats of the family on h: (the return code, the error text, n_dropped)."""
    c = (MapCounters if family == "map" else TsdfCounters)()
    r = (L.viso_map_stats if family == "map" else L.viso_tsdf_stats)(h, C.byref(c))
    return r, L.viso_last_error().decode(), int(c.n_dropped)


def _zero(outputs):
    return not any(bytes(o).strip(b"\0") for o in outputs)


def _run(L, rows, hs, expect, stats_of=None):
    """Every call of `rows` on its handles of hs (family "map": hs["map"]).  expect(family, name) is None for a call that must
    succeed, or (code, text behind "entry point: ").  Behind a refused call the outputs are zero and the stats of the handle
    (stats_of(family): the family whose stats the handle answers to; by default the call's) answer as before the call."""
    for family, name, kind, make in rows:
        entry = f"viso_{family}_{name}"
        for h in ([hs["map"]] if family == "map" else _handles(kind, hs)):
            stats_family = stats_of(family) if stats_of else family
            before = _stats(L, stats_family, h)
            call, outputs = make(h)
            r = call()
            got = L.viso_last_error().decode()
            want = expect(family, name)
            print(f"{entry}: {r} {got if r != OK else ''}")
            if want is None:
                assert r == OK, (entry, r, got)
                continue
            assert (r, got) == (want[0], f"{entry}: {want[1]}"), (entry, r, got)
            assert _zero(outputs), (entry, "a refused call wrote to its outputs")
            after = _stats(L, stats_family, h)
            assert after[0] == before[0] and after[2] == before[2], (entry, before, after)
            assert after[1] == before[1] or after[0] == OK, (entry, before, after)


def _not_live(family, name):
    return ARG, f"not a live {WORDS[family][0]} handle"


def test_destroyed_handle(viso):
    L = viso
    maps = _maps(None)
    hs = {which: t.h for which, t in maps.items()}
    for t in maps.values():
        t.close()
    for family in ("map", "tsdf"):
        r, text, _ = _stats(L, family, hs["map" if family == "map" else "plain"])
        assert r == ARG and text == f"viso_{family}_stats: not a live {WORDS[family][0]} handle"
    _run(L, _calls(L), hs, _not_live)


def test_live_handle_of_the_other_kind(viso):
    L = viso
    maps = _maps(None)
    # a voxel map for every TSDF call, a TSDF map for every call of the voxel map; the stats are those of the handle's own kind
    hs = {"map": maps["plain"].h, "plain": maps["map"].h, "gray": maps["map"].h}
    _run(L, _calls(L), hs, _not_live, stats_of=lambda family: "tsdf" if family == "map" else "map")
    assert maps["map"].count() == 0 and len(maps["plain"].entries()) == 0
    for t in maps.values():
        t.close()


def test_map_whose_context_was_destroyed(viso):
    L = viso
    ctx = libviso_amd.Context(0)
    maps = _maps(ctx)
    ctx.close()
    hs = {which: t.h for which, t in maps.items()}

    def expect(family, name):
        if (family, name) == ("tsdf", "is_gray"):   # asks the registry only
            return None
        return ARG, f"the {WORDS[family][1]}'s context has been destroyed"
    for family in ("map", "tsdf"):
        r, text, _ = _stats(L, family, hs["map" if family == "map" else "plain"])
        assert (r, text) == (ARG, f"viso_{family}_stats: the {WORDS[family][1]}'s context has been destroyed")
    _run(L, _calls(L), hs, expect)
    for t in maps.values():
        t.close()


def test_overflowed_map(viso):
    L = viso
    maps = _maps(None)
    _overflow(maps)
    hs = {which: t.h for which, t in maps.items()}
    rows = _calls(L)

    def expect(family, name):
        if name in NOT_REFUSING:
            return None
        _, noun, unit, clear_fn = WORDS[family]
        return NOMEM, (f"the {noun} has overflowed ({unit} were dropped; which ones depends on scheduling): {clear_fn} it, or use a larger "
                       "capacity_log2")
    for which, t in maps.items():
        assert t.stats()["n_dropped"] > 0, which
    _run(L, [row for row in rows if row[1] != "clear"], hs, expect)
    for which, t in maps.items():
        assert t.stats()["n_dropped"] > 0, which   # the refusals and the calls that answered left the mark
    # the clear, and after it every call
    _run(L, [row for row in rows if row[1] == "clear"], hs, lambda family, name: None)
    _run(L, rows, hs, lambda family, name: None)
    for t in maps.values():
        t.close()


def test_healthy_map(viso):
    L = viso
    maps = _maps(None)
    hs = {which: t.h for which, t in maps.items()}
    _run(L, _calls(L), hs, lambda family, name: None)
    for t in maps.values():
        t.close()
