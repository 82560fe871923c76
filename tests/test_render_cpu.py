"""The ray casting of the TSDF map (include/viso_hip.h, "TSDF render") without a device: the two numpy restatements
(tests/render_ref.py) against each other and against the scenes their input was made from, the refusals of the C ABI that touch no
device, the PNG writer of the tool and the kernel's resource usage."""
import ctypes as C

import numpy as np
import pytest

import libviso_amd
from libviso_amd import fuse_map, hostmath
from libviso_amd.abi import TSDF_ENTRY_DTYPE, Param

import render_ref as RR
import tsdf_ref as R
import tsdf_tables as TT
from estimator_util import kernel_resources

INV = R.INVALID
POSE = np.linalg.inv(hostmath.tr2mat([0.013, -0.021, 0.007, 0.31, -0.12, 1.47]))   # the pose of test_gpu_tsdf
SHAPE = (37, 333)


def _param():
    return Param.default(base=0.5371, f=721.5377, cu=609.5593, cv=172.854)


def _fused(name, shape=SHAPE, pose=POSE, voxel=0.2, trunc=3):
    e, st = R.fuse([(RR.scene_map(name, shape), pose)], _param(), voxel, trunc, 16)
    assert st["n_out_of_range"] == 0 and st["n_dropped"] == 0
    return e


@pytest.mark.parametrize("shape", [(3, 130), (1, 1)])
def test_the_two_restatements_agree(shape):
    prm = _param()
    n_valid = 0
    for i, name in enumerate(RR.SCENES):
        fuse_pose = (None, POSE)[i % 2]
        frames = [(RR.scene_map(name, shape, 0.1 if shape[1] > 1 else 0.0), fuse_pose)]
        frames.append((frames[0][0], RR.sideways(fuse_pose, 0.02)))
        e, st = R.fuse(frames, prm, 0.2, 3, 16)
        assert st["n_out_of_range"] == 0
        for view in (fuse_pose, RR.sideways(fuse_pose, 0.1, 0.01)):
            for mw in (1, 2):
                a = RR.render(e, 0.2, prm, shape, view, 17.0, mw)
                b = RR.render_loop(e, 0.2, prm, shape, view, 17.0, mw)
                assert a[0].dtype == b[0].dtype == np.int16 and a[1].dtype == b[1].dtype == np.uint32
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (name, mw)
                assert ((a[0] == INV) == (a[1] == 0)).all()
                n_valid += int((a[0] != INV).sum())
    assert n_valid > 0


def _both(case, tag, untraced=False):
    """The case by both restatements: equal bytes; (disparity, weight, trace).  untraced: also by the loop without a trace."""
    a = RR.render(*case)
    d, w, trace = TT.events(case)
    assert a[0].dtype == d.dtype == np.int16 and a[1].dtype == w.dtype == np.uint32
    assert a[0].tobytes() == d.tobytes() and a[1].tobytes() == w.tobytes(), tag
    assert ((d == INV) == (w == 0)).all() and set(trace) <= set(RR.EVENTS)
    if untraced:                                       # the trace changes nothing
        plain = RR.render_loop(*case)
        assert plain[0].tobytes() == d.tobytes() and plain[1].tobytes() == w.tobytes()
    return d, w, trace


def test_hand_built_tables_are_what_they_claim():
    """The cases of tests/tsdf_tables.py that aim at one event each (tests/test_gpu_render_edges.py runs them on the device)."""
    seen = {}
    for name, (fn, event) in TT.SMALL_CASES.items():
        d, w, trace = _both(fn(), name, untraced=True)
        print(f"{name}: {(d != INV).mean():.3f} valid, {dict(trace)}")
        assert trace[event] > 0, (name, dict(trace))
        seen[name] = (d, w, trace)
    d, w, t = seen["too_big"]
    assert (d == INV).all() and t["hit_too_big"] == t["hit"] == d.size == 45
    d, w, t = seen["too_big_alone"]
    assert (d == 3034).all() and (w == 2).all() and t["hit"] == 45 and t["hit_too_big"] == 0
    d, w, t = seen["too_small"]
    assert (d == INV).all() and t["hit_too_small"] == t["hit"] == 45
    d, w, t = seen["behind"]
    assert 0 < t["hit_behind"] < t["hit"] and (d != INV).any() and (d == INV).any()
    d, w, t = seen["gap_in"]
    assert (d == 7349).all() and t["gap"] == 45 * 12 and t["hit"] == 45                 # 0.3 m of gaps, a sample every 0.025 m
    d, w, t = seen["gap_out"]
    assert t["hit"] == (d != INV).sum() > 0 and (d[d != INV] == 13973).all() and (d == INV).any()
    assert t["gap"] == (d == INV).sum() * 81                                            # from 1 m to 3 m: samples 40 .. 120
    d, w, t = seen["gap_beside"]
    assert (d == INV).all() and t["hit"] == 0 and t["gap"] > 0 and set(t) == {"gap"}
    d, w, t = seen["weights_and_means"]
    assert set(np.unique(w).tolist()) == {0, 1, 2, 3, TT.BIG} and len(np.unique(d[d != INV])) >= 5


def test_random_block_sweeps_reach_every_event():
    """Every view of the two sweeps is between 5 % and 95 % valid, and over them every event of a ray through an irregular table
    occurs; first_negative only where the camera is inside the block."""
    total = {}
    for name in TT.BLOCKS:
        shares = []
        for pose, mw, case in TT.block_sweep(name):
            d, w, trace = _both(case, (name, pose, mw))
            shares.append(round(float((d != INV).mean()), 3))
            assert 0.05 <= shares[-1] <= 0.95, (name, pose, mw, shares[-1])
            assert (w[d != INV] >= mw).all()
            for k, v in trace.items():
                total[k] = total.get(k, 0) + v
            assert (trace["first_negative"] > 0) == (name == "inside")
        print(f"{name}: valid shares {shares}")
    print(total)
    for k in TT.BLOCK_EVENTS:
        assert total.get(k, 0) > 0, (k, total)
    for k in ("gap", "hit_too_big", "hit_too_small", "hit_behind"):
        assert total.get(k, 0) == 0
    for mw in TT.BLOCK_MIN_WEIGHTS:
        d, w, trace = _both(TT.chains_view(mw), ("chains", mw))
        assert 0.05 <= (d != INV).mean() <= 0.95 and trace["hit"] > 0


def test_table_builders():
    e = TT.slab(7, half=3, weight=2)
    assert len(e) == 2 * 36 and (np.diff(R.keys_of(e["k"])) > 0).all() and (e["weight"] == 2).all()
    assert (e["sum"][e["k"][:, 2] == 7] == 600).all() and (e["sum"][e["k"][:, 2] == 8] == -1000).all()
    assert e["k"][:, :2].min() == -3 and e["k"][:, :2].max() == 2
    a = TT.random_block(np.random.default_rng(9), origin=-4)
    b = TT.random_block(np.random.default_rng(9), origin=(-4, -4, -4))
    c = TT.random_block(np.random.default_rng(9), origin=(-4, 0, 3))
    assert a.tobytes() == b.tobytes() and len(a) == len(c) == 508
    assert np.array_equal(np.sort(c["k"] - (0, 4, 7), axis=0), np.sort(a["k"], axis=0))
    assert [len(R.crossings(a, mw)) for mw in (1, 2, 3)] == [485, 226, 47]
    lim = 3 * 1024 * a["weight"].astype(np.int64)
    assert (np.abs(a["sum"]) <= lim).all() and (a["sum"] == 0).any() and (a["sum"] == lim).any() and (a["sum"] == -lim).any()
    top = TT.crossing_block("top")
    assert ((top["k"] == R.BIAS - 1).any(axis=1)).sum() == 158


def test_fronto_parallel_wall_comes_back():
    """The wall (disparity 640) fused once from POSE at voxel 0.2 and T = 3, rendered from POSE at the same size.

    The bound.  Every pixel of the wall has the same Z = f base / 40, so every update of a voxel adds the same q = floor((Z - zc) / s)
    (step 6 of the map): da = (Z - za) / s - ea and db = (Z - zb) / s - eb with ea, eb in [0, 1), for the centre depths za, zb of
    the hit's two voxels.  da >= 0 > db gives za <= Z < zb, and t in [0, 1) gives za <= zs < zb, so |zs - Z| < zb - za = D s.
    With x = (Z - za) / s in [0, D): zs / s - za / s = D (x - ea) / (D - ea + eb), and its difference to x is
    -((D - x) ea + x eb) / (D - ea + eb), of magnitude below D / (D - 1) for D > 1.  min(D, D / (D - 1)) <= 2: |zs - Z| <= 2 s,
    whatever the two voxels are.  (The truncation does not interfere at T = 3: both voxels lie within one voxel diagonal of the
    surface.)  The rounding of the double operations is below 2^-40 s.  The value written is floor(16 f base / zs + 0.5), which is
    monotonic in zs: it lies between its values at Z + 2 s and Z - 2 s, the ends widened by 2^-30 Z for the rounding."""
    prm = _param()
    e = _fused("wall")
    d, w = RR.render(e, 0.2, prm, SHAPE, POSE, 20.0, 1)
    valid = d != INV
    Z, s = prm.f * prm.base / 40.0, 0.2 / 1024.0
    lo = int(np.floor(16.0 * prm.f * prm.base / ((Z + 2.0 * s) * (1.0 + 2.0 ** -30)) + 0.5))
    hi = int(np.floor(16.0 * prm.f * prm.base / ((Z - 2.0 * s) * (1.0 - 2.0 ** -30)) + 0.5))
    print(f"wall: {valid.mean():.3f} valid, values {np.unique(d[valid]).tolist()}, bound {lo} .. {hi}, weights {w[valid].min()} .. {w.max()}")
    assert (lo, hi) == (640, 640)          # 2 s of depth are 0.026 sixteenths of a pixel at 40 px
    assert valid.mean() > 0.5 and (d[valid] >= lo).all() and (d[valid] <= hi).all() and (w[valid] >= 1).all()
    # seen from behind: the camera turned by 180 degrees about its vertical axis, twice the wall's depth away and moved sideways so
    # that it looks back at the part of the wall that was seen.  Only front-to-back crossings count: nothing.
    Xc = (SHAPE[1] / 2.0 - prm.cu) / prm.f * Z
    back = np.eye(4)
    back[0, 0], back[2, 2], back[0, 3], back[2, 3] = -1.0, -1.0, 2.0 * Xc, 2.0 * Z
    d2, w2 = RR.render(e, 0.2, prm, SHAPE, POSE @ back, 20.0, 1)
    assert (d2 == INV).all() and not w2.any()
    # the rays do cross the wall: with every sign reversed the same view sees a surface
    neg = e.copy()
    neg["sum"] = -neg["sum"] - 1
    d3, _ = RR.render(neg, 0.2, prm, SHAPE, POSE @ back, 20.0, 1)
    assert (d3 != INV).mean() > 0.5


# Measured on the restatement (vectorised, voxel 0.2, T = 3, fused from POSE at 37 x 333, max_depth 20, min_weight 1): the largest and
# the median absolute difference to the analytically rendered disparity over the pixels where both are valid, in sixteenths of a
# pixel.  They describe the method (the nearest voxel, projective distances), not an error of the code; DESIGN.md 5.17 has them.
# The step seen from the fusing pose: 240 = 15 px is the whole step, at the pixels beside the edge whose rays enter a voxel that
# the near half filled before they reach the far half (the nearest voxel bleeds by up to a voxel's footprint).
MEASURED = {("plane", "same"): (5.00, 1.20), ("plane", "moved"): (4.93, 1.20), ("step", "same"): (240.0, 0.0), ("step", "moved"): (0.0, 0.0)}


@pytest.mark.parametrize("name", ["plane", "step"])
def test_slanted_plane_and_depth_step_against_the_analytic_render(name):
    prm = _param()
    e = _fused(name)
    for tag, view in (("same", POSE), ("moved", RR.sideways(POSE, 0.5))):
        d, _ = RR.render(e, 0.2, prm, SHAPE, view, 20.0, 1)
        want = RR.ideal(name, SHAPE, prm, POSE, view)
        both = (d != INV) & np.isfinite(want)
        err = np.abs(d[both].astype(np.float64) - want[both] * 16.0)
        print(f"{name}, {tag}: {(d != INV).mean():.3f} valid, {int(both.sum())} compared, max {err.max():.2f}, median {np.median(err):.2f} sixteenths")
        assert both.mean() > 0.5
        assert err.max() <= MEASURED[name, tag][0] + 1.0 and np.median(err) <= MEASURED[name, tag][1] + 1.0


def test_nothing_to_see():
    prm = _param()
    e = _fused("wall", (3, 130))
    for entries, mw in ((np.zeros(0, TSDF_ENTRY_DTYPE), 1), (e, int(e["weight"].max()) + 1)):
        for fn in (RR.render, RR.render_loop):
            d, w = fn(entries, 0.2, prm, (3, 130), POSE, 17.0, mw)
            assert d.shape == w.shape == (3, 130) and (d == INV).all() and not w.any()
    assert (RR.render(e, 0.2, prm, (3, 130), POSE, 17.0, 1)[0] != INV).any()


def test_frame_order_does_not_matter():
    prm = _param()
    a, b = (RR.scene_map("step", (3, 130)), POSE), (RR.scene_map("plane", (3, 130)), RR.sideways(POSE, 0.05))
    e1, _ = R.fuse([a, b], prm, 0.2, 3, 16)
    e2, _ = R.fuse([b, a], prm, 0.2, 3, 16)
    r1, r2 = RR.render(e1, 0.2, prm, (3, 130), POSE, 17.0, 2), RR.render(e2, 0.2, prm, (3, 130), POSE, 17.0, 2)
    assert r1[0].tobytes() == r2[0].tobytes() and r1[1].tobytes() == r2[1].tobytes() and (r1[0] != INV).any()


def test_symbol_is_declared_and_exported():
    L = libviso_amd.load()
    assert len(L.viso_tsdf_render.argtypes) == 10 and L.viso_tsdf_render.argtypes[5] is C.c_double
    assert callable(libviso_amd.TsdfMap.render)


def test_argument_errors_without_a_device():
    """What does not need the map is checked before the handle: every such error answers with VISO_ERR_ARG and "bad argument"
    whatever the handle is, and follows no pointer of it.  With good arguments a handle that is not a live TSDF map is refused."""
    L = libviso_amd.load()
    prm = _param()
    d = np.full((2, 2, 3), 77, np.int16)
    w = np.full((2, 2, 3), 77, np.uint32)
    T = np.stack([np.eye(4), POSE])
    dp, wp, Tp = d.ctypes.data_as(C.POINTER(C.c_int16)), w.ctypes.data_as(C.POINTER(C.c_uint32)), T.ctypes.data_as(C.POINTER(C.c_double))

    def call(handle, min_weight=1, param=prm, rows=2, cols=3, max_depth=10.0, poses=Tp, n_views=2, out=dp):
        return L.viso_tsdf_render(handle, min_weight, C.byref(param) if param is not None else None, rows, cols, max_depth, poses, n_views, out, wp)

    def bad_param(**kw):
        p = _param()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    Tbad = T.copy()
    Tbad[1, 2, 3] = np.inf
    wrong = [dict(min_weight=0), dict(param=None), dict(out=None), dict(rows=0), dict(cols=0), dict(rows=-1), dict(rows=65536, cols=65536),
             dict(max_depth=0.0), dict(max_depth=-1.0), dict(max_depth=np.inf), dict(max_depth=np.nan), dict(n_views=0), dict(n_views=-3),
             dict(poses=None, n_views=2), dict(poses=Tbad.ctypes.data_as(C.POINTER(C.c_double))),
             dict(param=bad_param(f=0.0)), dict(param=bad_param(f=-1.0)), dict(param=bad_param(base=0.0)), dict(param=bad_param(f=np.nan)),
             dict(param=bad_param(cu=np.inf)), dict(param=bad_param(cv=np.nan)), dict(param=bad_param(base=np.inf))]
    for handle in (None, C.c_void_p(4096)):
        for kw in wrong:
            assert call(handle, **kw) == -1, kw
            msg = L.viso_last_error()
            assert b"viso_tsdf_render" in msg and b"bad argument" in msg, (kw, msg)
        assert call(handle) == -1
        assert b"viso_tsdf_render: not a live TSDF handle" in L.viso_last_error()
        assert call(handle, poses=None, n_views=1) == -1 and b"not a live" in L.viso_last_error()
    assert (d == 77).all() and (w == 77).all()
    # a handle of the other kind of map is foreign too; the Python method raises with the code
    m = object.__new__(libviso_amd.TsdfMap)
    m.L, m.h = L, 4096
    try:
        with pytest.raises(libviso_amd.VisoError, match="-1"):
            m.render(prm, (2, 3))
        with pytest.raises(ValueError):
            m.render(prm, (2, 3), poses=np.eye(3))
        with pytest.raises(ValueError):
            m.render(prm, (0, 3))
    finally:
        m.h = None


def test_disparity_png_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (7, 13)):
        m = rng.integers(1, 4096, shape).astype(np.int16)
        m[rng.random(shape) < 0.3] = INV
        m.flat[0] = 4095                      # 4095 x 16 = 65520: the largest value a file holds
        f = str(tmp_path / "m.png")
        fuse_map.write_disparity_png(f, m)
        back = fuse_map.read_disparity_png(f)
        assert back.dtype == np.int16 and back.tobytes() == m.tobytes()
    with pytest.raises(ValueError):
        fuse_map.write_disparity_png(str(tmp_path / "bad.png"), np.zeros((2, 2), np.int16))


def test_tool_refuses_render_without_a_tsdf_map(capsys):
    with pytest.raises(SystemExit) as ex:
        fuse_map.main(["maps", "poses.txt", "calib.txt", "out.ply", "--render", "views"])
    assert ex.value.code == 2 and "--render needs" in capsys.readouterr().err


def test_render_kernel_has_no_scratch():
    res = kernel_resources("tsdf.hip", ("tsdf_render_kernel",))
    occ, scratch = res["tsdf_render_kernel"]
    print(f"tsdf_render_kernel: occupancy {occ}, scratch {scratch}")
    assert scratch == 0 and occ >= 1
