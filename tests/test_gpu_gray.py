"""The gray TSDF map on the device (include/viso_hip.h, "TSDF intensity"; libviso_amd/csrc/tsdf.hip) against its numpy restatement
(tests/gray_ref.py), byte for byte, and against the plain map fused from the same input.

Input condition of the bit-exact tests, as in tests/test_gpu_tsdf.py: the restatement itself reports n_out_of_range == 0 and
n_dropped == 0 (asserted first).  The deliberate overflow case is the exception."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd import hostmath, synth
from libviso_amd.abi import TSDF_GRAY_ENTRY_DTYPE, TSDF_MESH_VERTEX_DTYPE, MatchParams

import gray_cases as GC
import gray_ref as G
import render_ref as RR
import tsdf_ref as R
import tsdf_tables as TT
from test_gpu_tsdf import _mixed_map

pytestmark = pytest.mark.gpu

INV = R.INVALID
POSE = GC.POSE
LOG2 = 21


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _clean(st):
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0, st
    return st


def _image(rng, shape):
    im = rng.integers(0, 256, shape).astype(np.uint8)
    im.flat[0], im.flat[-1] = 0, 255
    return im


def _gray_map(ctx=None, **kw):
    t = libviso_amd.TsdfMap(ctx, gray=True, **kw)
    kind = C.c_int(-1)
    assert t.gray and t.L.viso_tsdf_is_gray(t.h, C.byref(kind)) == 1 and kind.value == 1
    return t


def _check_against_plain(gray, plain, prm, shape, pose, tag):
    """The unchanged readers of a gray map give what they give for the plain map fused from the same input."""
    assert gray.stats() == plain.stats(), tag
    assert _same(gray.entries(), plain.entries()) and _same(gray.entries(2), plain.entries(2)), tag
    assert gray.L.viso_tsdf_count(gray.h, 1, C.byref(C.c_size_t())) == 1
    assert _same(gray.surface(), plain.surface()), tag
    (gv, gt), (pv, pt) = gray.mesh(), plain.mesh()
    assert _same(gv, pv) and _same(gt, pt), tag
    for a, b in zip(gray.render(prm, shape, pose, max_depth=30.0, min_weight=1, weights=True),
                    plain.render(prm, shape, pose, max_depth=30.0, min_weight=1, weights=True)):
        assert _same(a, b), tag
    return gv


# ---- 1. the device equals the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 130), (1, 1), (37, 333)])
@pytest.mark.parametrize("trunc", [1, 8])
def test_device_equals_restatement(viso, shape, trunc):
    rng = np.random.default_rng(shape[0] * 5 + shape[1] + trunc)
    m = _mixed_map(rng, *shape) if shape != (1, 1) else np.array([[400]], np.int16)
    if m.size > 1:
        m[0, 60:70] = 200            # one run across the first wave boundary
    im = _image(rng, shape) if m.size > 1 else np.array([[255]], np.uint8)
    prm = GC.param()
    n_cross = 0
    for voxel in (0.05, 0.2, 5.0):
        gray = _gray_map(voxel=voxel, trunc_voxels=trunc, capacity_log2=LOG2)
        plain = libviso_amd.TsdfMap(None, voxel=voxel, trunc_voxels=trunc, capacity_log2=LOG2)
        assert not plain.gray
        for name, pose in (("none", None), ("rigid", POSE)):
            tag = (shape, trunc, voxel, name)
            want, st = G.fuse([(m, im, pose)], prm, voxel, trunc, 16, LOG2)
            _clean(st)
            gray.clear(); plain.clear()
            gray.fuse(m, prm, pose=pose, image=im)
            plain.fuse(m, prm, pose=pose)
            e = gray.entries(gray=True)
            assert e.dtype == TSDF_GRAY_ENTRY_DTYPE == G.ENTRY and _same(e, want), tag
            assert _same(gray.entries(2, gray=True), want[want["weight"] >= 2]), tag
            assert gray.stats() == st, tag
            v = _check_against_plain(gray, plain, prm, shape, pose, tag)
            c = gray.surface()                                     # (a map of one view has few complete cells: the crossings too)
            for edges in (v, G.crossing_vertices(c)):
                g, missing = gray.vertex_gray(edges, missing=True)
                wg, wm = G.vertex_gray(want, edges)
                assert _same(g, wg) and missing == wm == 0, tag
            assert _same(gray.vertex_gray(c), wg), tag
            n_cross += len(c)
        gray.close(); plain.close()
    assert n_cross > 0 or m.size == 1


def test_a_full_wave_as_one_run(viso):
    """All pixels at one disparity, an all-255 image, voxel 5.0, trunc 8: every wave of a row is one run of 64 lanes, so the run's
    sum of q and its sum of intensities are both the largest a run can have (64 x 255 = 16320)."""
    m = np.full((3, 130), 200, np.int16)
    im = np.full((3, 130), 255, np.uint8)
    prm = GC.param()
    for pose in (None, POSE):
        want, st = G.fuse([(m, im, pose)], prm, 5.0, 8, 16, LOG2)
        _clean(st)
        assert (want["gray"] == 255 * want["weight"].astype(np.uint64)).all() and want["weight"].max() >= 64
        t = _gray_map(voxel=5.0, trunc_voxels=8, capacity_log2=LOG2)
        t.fuse(m, prm, pose=pose, image=im)
        assert _same(t.entries(gray=True), want) and t.stats() == st
        t.close()


# ---- 2. order and additivity ------------------------------------------------------------------------------------------------------
def test_order_additivity_and_clear(viso):
    rng = np.random.default_rng(31)
    prm = GC.param()
    frames = [(_mixed_map(rng, 20, 150), _image(rng, (20, 150)), p) for p in (None, POSE, POSE @ POSE, np.linalg.inv(POSE))]
    want, st = G.fuse(frames, prm, capacity_log2=LOG2)
    _clean(st)
    a, b, c = (_gray_map(capacity_log2=LOG2) for _ in range(3))
    for m, im, p in frames:
        a.fuse(m, prm, pose=p, image=im)
    for m, im, p in frames[::-1]:
        b.fuse(m, prm, pose=p, image=im)
    assert _same(a.entries(gray=True), want) and _same(b.entries(gray=True), want) and a.stats() == st == b.stats()
    # two maps over disjoint frames, joined by add_gray_entries
    b.clear()
    for m, im, p in frames[:1]:
        b.fuse(m, prm, pose=p, image=im)
    for m, im, p in frames[1:]:
        c.fuse(m, prm, pose=p, image=im)
    part_b, part_c = b.entries(gray=True), c.entries(gray=True)
    assert _same(part_b, G.fuse(frames[:1], prm, capacity_log2=LOG2)[0]) and _same(G.merge(part_b, part_c), want)
    b.add_entries(part_c)
    assert _same(b.entries(gray=True), want)
    assert b.stats()["n_updates"] == st["n_updates"] and b.stats()["n_occupied"] == st["n_occupied"]
    # fuse, clear, fuse another map: the second alone, so gray was cleared
    second, st2 = G.fuse(frames[2:3], prm, capacity_log2=LOG2)
    a.clear()
    assert len(a.entries(gray=True)) == 0 and a.stats()["n_occupied"] == 0
    a.fuse(frames[2][0], prm, pose=frames[2][2], image=frames[2][1])
    assert _same(a.entries(gray=True), second) and a.stats() == st2
    for t in (a, b, c):
        t.close()


# ---- 3. refusals -----------------------------------------------------------------------------------------------------------------
def _refused(code, fn, *args, **kw):
    with pytest.raises(libviso_amd.VisoError, match=f"with {code}:"):
        fn(*args, **kw)


def test_kinds_do_not_mix(viso):
    rng = np.random.default_rng(41)
    prm = GC.param()
    m, im = _mixed_map(rng, 10, 70), _image(rng, (10, 70))
    gray, plain = _gray_map(capacity_log2=LOG2), libviso_amd.TsdfMap(None, capacity_log2=LOG2)
    gray.fuse(m, prm, image=im)
    plain.fuse(m, prm)
    ge, pe = gray.entries(gray=True), plain.entries()
    gst, pst = gray.stats(), plain.stats()
    v = plain.mesh()[0][:5]
    L = gray.L
    mp, ip = m.ctypes.data_as(C.POINTER(C.c_int16)), im.ctypes.data_as(C.POINTER(C.c_uint8))
    n = C.c_size_t()
    out_d, out_g = np.zeros(m.shape, np.int16), np.zeros(m.shape, np.uint8)
    dp, gp = out_d.ctypes.data_as(C.POINTER(C.c_int16)), out_g.ctypes.data_as(C.POINTER(C.c_uint8))
    # the plain calls on a gray map
    assert L.viso_tsdf_fuse(gray.h, mp, 10, 70, C.byref(prm), None) == -1 and b"viso_tsdf_fuse" in L.viso_last_error()
    assert L.viso_tsdf_add_entries(gray.h, pe.ctypes.data, len(pe)) == -1
    with pytest.raises(ValueError):
        gray.fuse(m, prm)
    _refused(-1, gray.add_entries, pe)
    # the gray calls on a plain map
    assert L.viso_tsdf_fuse_gray(plain.h, mp, ip, 10, 70, C.byref(prm), None) == -1
    assert L.viso_tsdf_add_gray_entries(plain.h, ge.ctypes.data, len(ge)) == -1
    assert L.viso_tsdf_get_gray(plain.h, 1, ge.ctypes.data, len(ge), C.byref(n)) == -1
    assert L.viso_tsdf_vertex_gray(plain.h, v.ctypes.data, len(v), gp, C.byref(n)) == -1
    assert L.viso_tsdf_render_gray(plain.h, 1, C.byref(prm), 10, 70, 30.0, None, 1, dp, None, gp) == -1
    with pytest.raises(ValueError):
        plain.fuse(m, prm, image=im)
    _refused(-1, plain.add_entries, ge)
    _refused(-1, plain.entries, gray=True)
    _refused(-1, plain.vertex_gray, v)
    _refused(-1, plain.mesh, gray=True)
    _refused(-1, plain.render, prm, m.shape, gray=True)
    kind = C.c_int(-1)
    assert L.viso_tsdf_is_gray(plain.h, C.byref(kind)) == 1 and kind.value == 0 and L.viso_tsdf_is_gray(plain.h, None) == -1
    # a null image, a wrong image, a gray sum beyond 255 weight
    assert L.viso_tsdf_fuse_gray(gray.h, mp, None, 10, 70, C.byref(prm), None) == -1 and b"image" in L.viso_last_error()
    for bad in (im[:, :-1], im.astype(np.uint16), im[0]):
        with pytest.raises(ValueError):
            gray.fuse(m, prm, image=bad)
    big = ge[:3].copy()
    big["gray"][1] = 255 * int(big["weight"][1]) + 1
    _refused(-1, gray.add_entries, big)
    for field, value in (("weight", 0), ("sum", 4 * 1024 * 10 ** 6), ("k", R.BIAS)):
        bad = ge[:3].copy()
        bad[field][2] = value
        _refused(-1, gray.add_entries, bad)
    assert L.viso_tsdf_render_gray(gray.h, 1, C.byref(prm), 10, 70, 30.0, None, 1, dp, None, None) == -1
    # nothing of all that touched either table
    assert _same(gray.entries(gray=True), ge) and _same(plain.entries(), pe) and gray.stats() == gst and plain.stats() == pst
    gray.close(); plain.close()
    assert L.viso_tsdf_is_gray(gray.h, C.byref(kind)) == -1


def test_overflow_and_recovery(viso):
    rng = np.random.default_rng(43)
    prm = GC.param()
    m, im = _mixed_map(rng, 37, 333), _image(rng, (37, 333))
    assert len(G.fuse([(m, im, None)], prm, 0.2, 3, 16, 10)[0]) > 1024
    t = _gray_map(capacity_log2=10)
    _refused(-4, t.fuse, m, prm, image=im)
    assert t.stats()["n_dropped"] > 0
    v = np.zeros(1, TSDF_MESH_VERTEX_DTYPE); v["dir"] = 1
    one = np.zeros(1, TSDF_GRAY_ENTRY_DTYPE); one["weight"] = 1
    for fn, args, kw in ((t.entries, (), dict(gray=True)), (t.vertex_gray, (v,), {}), (t.mesh, (), dict(gray=True)),
                         (t.render, (prm, (4, 5)), dict(gray=True)), (t.add_entries, (one,), {}), (t.fuse, (m, prm), dict(image=im))):
        _refused(-4, fn, *args, **kw)
    t.clear()
    small, sim = m[:2, :40], np.ascontiguousarray(im[:2, :40])
    want, st = G.fuse([(small, sim, None)], prm, 0.2, 3, 16, 10)
    assert st["n_dropped"] == 0 and 0 < len(want) <= 1024
    t.fuse(small, prm, image=sim)
    assert _same(t.entries(gray=True), want) and t.stats() == st
    t.close()


# ---- 4. the resident path ---------------------------------------------------------------------------------------------------------
def test_resident_path(viso):
    seq = synth.make_subpixel_image_sequence(4, 6, n_kp=500, width=640, height=200)
    prm = seq["param"]
    ctx = libviso_amd.Context(0)
    nf, cap = seq["kp"].shape[0], seq["kp"].shape[2]
    b = libviso_amd.Batch(ctx, nf, cap)
    b.upload_images(seq["images"], seq["kp"], seq["n"])
    b.set_params(MatchParams.stereo(seq["F"]), MatchParams.temporal(), seq["param"], seed=3)
    b.set_disparity(num_disp=64)
    b.run_images()
    tr, ok, n_inl = b.poses()
    poses, valid = hostmath.chain_poses(tr, ok)
    assert len(valid) >= 2
    T = np.tile(np.eye(4), (nf, 1, 1))
    for k, t in enumerate(valid):
        T[t] = poses[k + 1]
    maps, lefts = b.disparities(), np.stack([b.image(t, 0) for t in range(nf)])
    rights = np.stack([b.image(t, 1) for t in range(nf)])
    assert (maps != INV).mean() > 0.2 and lefts.std() > 5 and np.array_equal(lefts, seq["images"][:, 0])
    want, st = G.fuse([(maps[t], lefts[t], T[t]) for t in range(nf)], prm, capacity_log2=LOG2)
    _clean(st)
    # the resident fuse, all frames in one call ...
    whole = _gray_map(ctx, capacity_log2=LOG2)
    b.fuse_tsdf(whole, T)
    assert _same(whole.entries(gray=True), want) and whole.stats() == st
    # ... equals the host path over the downloaded images and maps
    host = _gray_map(None, capacity_log2=LOG2)
    for t in reversed(range(nf)):
        host.fuse(maps[t], prm, pose=T[t], image=lefts[t])
    assert _same(host.entries(gray=True), want) and host.stats() == st
    # ... and a split into two frame ranges
    split = _gray_map(ctx, capacity_log2=LOG2)
    b.fuse_tsdf(split, T[2:], t0=2)
    assert _same(split.entries(gray=True), G.fuse([(maps[t], lefts[t], T[t]) for t in range(2, nf)], prm, capacity_log2=LOG2)[0])
    b.fuse_tsdf(split, T[:2], t0=0, t1=2)
    assert _same(split.entries(gray=True), want) and split.stats() == st
    # a plain map through the same call is the plain map
    plain = libviso_amd.TsdfMap(ctx, capacity_log2=LOG2)
    b.fuse_tsdf(plain, T)
    assert _same(plain.entries(), G.plain(want)) and plain.stats() == st
    # the batch's own outputs are what they were
    tr2, ok2, n_inl2 = b.poses()
    assert _same(tr2, tr) and _same(ok2, ok) and _same(n_inl2, n_inl) and _same(b.disparities(), maps)
    assert _same(np.stack([b.image(t, 0) for t in range(nf)]), lefts) and _same(np.stack([b.image(t, 1) for t in range(nf)]), rights)
    # a map of another context is refused, and the map is untouched
    with pytest.raises(libviso_amd.VisoError, match="-1"):
        b.fuse_tsdf(host, T)
    assert _same(host.entries(gray=True), want)
    for t in (whole, host, split, plain):
        t.close()
    b.close(); ctx.close()


# ---- 5. vertex_gray and 6. render_gray on random blocks -----------------------------------------------------------------------------
def _gray_block(name, seed=0):
    """The random block of tests/tsdf_tables.py with random gray sums: a tenth each at 0 and at 255 weight."""
    e = TT.block_entries(name)
    rng = np.random.default_rng(100 + seed)
    w = e["weight"].astype(np.int64)
    g = rng.integers(0, 255 * w + 1)
    special = rng.integers(0, 10, len(e))
    g = np.where(special == 0, 0, np.where(special == 1, 255 * w, g))
    return G.with_gray(e, g)


def _loaded(entries, voxel, log2=13):
    t = _gray_map(voxel=voxel, capacity_log2=log2)
    t.add_entries(entries)
    assert _same(t.entries(gray=True), entries)
    return t


@pytest.mark.parametrize("name", list(TT.BLOCKS))
def test_vertex_gray_on_random_blocks(viso, name):
    e = _gray_block(name)
    t = _loaded(e, 0.2)
    n_vert = 0
    for mw in TT.BLOCK_MIN_WEIGHTS:                                # (few cells are complete at 2, none at 3: the crossings remain)
        v, tri, g = t.mesh(mw, gray=True)
        want, missing = G.vertex_gray(e, v)
        assert _same(g, want) and missing == 0, (name, mw)
        c = t.surface(mw)
        gc, mc = t.vertex_gray(c, missing=True)
        want_c, wm = G.vertex_gray(e, G.crossing_vertices(c))
        assert _same(gc, want_c) and mc == wm == 0 and len(c) > 50 and len(set(gc.tolist())) > 30, (name, mw)
        # a crossing is the mesh's vertex of dir 1 << axis
        both = {(tuple(x["k"].tolist()), int(x["dir"])): int(y) for x, y in zip(v, g)}
        hits = [both.get((tuple(x["k"].tolist()), 1 << int(x["axis"]))) for x in c]
        assert all(h is None or h == int(y) for h, y in zip(hits, gc)) and (mw > 1 or sum(h is not None for h in hits) > 10)
        n_vert += len(v)
    assert n_vert > 50
    # every (k, dir) of the block's bounding box and a layer around it: absent ends and ends of one sign are missing, with 0
    (lo, hi) = e["k"].min(axis=0) - 1, e["k"].max(axis=0) + 1
    grid = np.stack(np.meshgrid(*[np.arange(a, b + 1) for a, b in zip(lo, hi)], np.arange(1, 8), indexing="ij"), axis=-1).reshape(-1, 4)
    every = np.zeros(len(grid), TSDF_MESH_VERTEX_DTYPE)
    every["k"], every["dir"] = grid[:, :3], grid[:, 3]
    g, missing = t.vertex_gray(every, missing=True)
    want, wm = G.vertex_gray(e, every)
    assert _same(g, want) and missing == wm and 0 < missing < len(every) and (g != 0).sum() > 100, (name, missing, len(every))
    print(f"{name}: {len(every)} edges, {missing} without a value")
    # nothing, and the refusals of the range
    g, missing = t.vertex_gray(every[:0], missing=True)
    assert len(g) == 0 and missing == 0
    for k, d in (((0, 0, 0), 0), ((0, 0, 0), 8), ((0, 0, 0), -1), ((R.BIAS - 1, 0, 0), 1), ((0, R.BIAS - 1, 0), 6), ((0, 0, R.BIAS - 1), 4),
                 ((-R.BIAS - 1, 0, 0), 2), ((0, R.BIAS, 0), 1)):
        bad = every[:3].copy()
        bad["k"][1], bad["dir"][1] = k, d
        assert not G.vertex_ok(bad).all()
        _refused(-1, t.vertex_gray, bad)
    edge = np.zeros(2, TSDF_MESH_VERTEX_DTYPE)
    edge["k"], edge["dir"] = [[R.BIAS - 1, R.BIAS - 2, -R.BIAS], [R.BIAS - 2, R.BIAS - 2, R.BIAS - 2]], [2, 7]
    g, missing = t.vertex_gray(edge, missing=True)                 # the last voxels that have a neighbour: accepted, absent
    assert g.tolist() == [0, 0] and missing == 2
    t.close()


@pytest.mark.parametrize("name", list(TT.BLOCKS))
def test_render_gray_on_random_blocks(viso, name):
    e = _gray_block(name, 1)
    sweep = TT.block_sweep(name)
    t = _loaded(e, 0.2)
    plain = libviso_amd.TsdfMap(None, voxel=0.2, capacity_log2=13)
    plain.add_entries(G.plain(e))
    for pose, mw, case in sweep:
        _, voxel, prm, shape, T, max_depth, _ = case
        want = G.render(e, voxel, prm, shape, T, max_depth, mw)
        assert len(set(want[2][want[0] != INV].tolist())) >= 8, (name, pose, mw)   # the input condition: no view of one shade
        got = t.render(prm, shape, T, max_depth=max_depth, min_weight=mw, weights=True, gray=True)
        assert len(got) == 3 and all(_same(a, b) for a, b in zip(got, want)), (name, pose, mw)
        assert _same(t.render(prm, shape, T, max_depth=max_depth, min_weight=mw, gray=True)[1], want[2])
        for a, b in zip(got[:2], plain.render(prm, shape, T, max_depth=max_depth, min_weight=mw, weights=True)):
            assert _same(a, b), (name, pose, mw)
        assert (got[2][got[0] == INV] == 0).all()
    # several views in one call, both pose forms
    names = TT.BLOCKS[name][7]
    _, voxel, prm, shape, _, max_depth, _ = sweep[0][2]
    views = np.stack([np.eye(4) if TT.BLOCK_POSES[p] is None else TT.BLOCK_POSES[p] for p in names] * 2)
    d, w, g = t.render(prm, shape, views, max_depth=max_depth, min_weight=1, weights=True, gray=True)
    assert d.shape == (len(views),) + tuple(shape) == g.shape and g.dtype == np.uint8
    for i, T in enumerate(views):
        one = t.render(prm, shape, T, max_depth=max_depth, min_weight=1, weights=True, gray=True)
        assert _same(d[i], one[0]) and _same(w[i], one[1]) and _same(g[i], one[2])
        assert _same(g[i], G.render(e, voxel, prm, shape, T, max_depth, 1)[2])
    if "none" in names:
        assert _same(t.render(prm, shape, None, max_depth=max_depth, min_weight=1, gray=True)[1], g[names.index("none")])
    t.close(); plain.close()


@pytest.mark.parametrize("name,pose", GC.CASES)
def test_known_answers_on_walls(viso, name, pose):
    """The known answers of tests/test_gray_cpu.py once more, on the device's own fuse, mesh and render."""
    m, voxel, max_depth, Z = GC.wall(name)
    T, prm, w = GC.POSES[pose], GC.param(), GC.window(name)
    t = _gray_map(voxel=voxel, trunc_voxels=GC.TRUNC, capacity_log2=LOG2)
    for tag, im in GC.images().items():
        t.clear()
        t.fuse(m, prm, pose=T, image=im)
        assert t.stats()["n_out_of_range"] == 0 and t.stats()["n_dropped"] == 0
        e = t.entries(gray=True)
        d, g = t.render(prm, GC.SHAPE, T, max_depth=max_depth, min_weight=1, gray=True)
        worst = GC.check_render(f"{name}/{pose}/{tag}", im, w, d, g)
        v, _, gv = t.mesh(1, gray=True)
        assert len(v) > 0
        if tag == "const":
            c = int(im.flat[0])
            assert (e["gray"] == np.uint64(c) * e["weight"].astype(np.uint64)).all()
            assert (gv == c).all() and (g[d != INV] == c).all() and worst == 0
        else:
            assert int(gv.min()) >= int(im.min()) and int(gv.max()) <= int(im.max())
    t.close()


# ---- 7. the tool --------------------------------------------------------------------------------------------------------------------
def test_fuse_map_gray(viso, tmp_path):
    """python -m libviso_amd.fuse_map --mesh --gray IMAGE_DIR --render DIR against the methods it is made of."""
    from libviso_amd import fuse_map
    rng = np.random.default_rng(51)
    prm = GC.param()
    names = ["%06d.png" % i for i in (4, 5)]
    T = [np.eye(4), RR.sideways(None, 0.05, 0.0)]
    maps = [np.full((40, 130), 400, np.int16), np.full((40, 130), 416, np.int16)]
    maps[1][:, 100:] = INV
    ims = [_image(rng, (40, 130)), GC.images()["ramp"]]
    d, g, views = tmp_path / "disp", tmp_path / "image_0", tmp_path / "views"
    d.mkdir(); g.mkdir()
    for n, m, im in zip(names, maps, ims):
        fuse_map.write_disparity_png(str(d / n), m)
        fuse_map.write_png8(str(g / n), im)
    (tmp_path / "poses.txt").write_text("".join(" ".join(repr(float(v)) for v in P[:3].reshape(-1)) + "\n" for P in T))
    (tmp_path / "calib.txt").write_text("P0: %r 0 %r 0 0 %r %r 0 0 0 1 0\nP1: %r 0 %r %r 0 %r %r 0 0 0 1 0\n" % (
        prm.f, prm.cu, prm.f, prm.cv, prm.f, prm.cu, -prm.f * prm.base, prm.f, prm.cv))
    ply = tmp_path / "m.ply"
    args = [str(d), str(tmp_path / "poses.txt"), str(tmp_path / "calib.txt"), str(ply), "--mesh", "--capacity-log2", "20"]
    assert fuse_map.main(args + ["--gray", str(g), "--render", str(views), "--render-depth", "20"]) == 0
    f, cu, cv, base = fuse_map.read_calib(str(tmp_path / "calib.txt"))
    prm = type(prm).default(base=base, f=f, cu=cu, cv=cv)
    T = fuse_map.read_poses(str(tmp_path / "poses.txt"))
    t = _gray_map(capacity_log2=20)
    for m, im, P in zip(maps, ims, T):
        t.fuse(m, prm, pose=P, image=im)
    v, tri, gv = t.mesh(1, gray=True)
    assert len(tri) > 100 and ply.read_bytes() == libviso_amd.mesh_ply_bytes(v, tri, gv) == G.mesh_ply_bytes(v, tri, gv)
    want_d, want_g = t.render(prm, (40, 130), T, max_depth=20.0, min_weight=1, gray=True)
    t.close()
    for i, n in enumerate(names):
        assert _same(fuse_map.read_disparity_png(str(views / n)), want_d[i]) and _same(fuse_map.read_png8(str(views / "gray" / n)), want_g[i])
    assert (want_d != INV).sum() > 5000 and len(set(want_g.reshape(-1).tolist())) > 50
    # without --gray the tool writes today's file
    assert fuse_map.main(args) == 0
    assert ply.read_bytes() == libviso_amd.mesh_ply_bytes(v, tri)
    with pytest.raises(SystemExit):
        fuse_map.main(args[:4] + ["--gray", str(g)])
