"""The direct calls (a batch stage's kernel on host pointers: DirectCall, libviso_amd/csrc/common.h) share the default context's
scratch blocks with each other and with the plain family (ScratchSlot): any order of calls must give every call its own answer.

Each order runs in a fresh child process, so that the blocks start empty and ctx_scratch really grows them: every call at a small
size (block allocated), a large one (more than 1.5 times the bytes: reallocated), and the small one again (an oversized block
reused).  The child only saves what the calls returned; this process compares the arrays with the models the per-feature tests
use (the oracle, tests/*_ref.py), with those tests' own comparisons.  A short per-call frame loop of the plain family runs next
to viso_detect_harris_binned and viso_support_sizes, which also run BETWEEN its calls -- they take the hypothesis slots of the
RANSAC stage the frame's stereo call has left running -- and must give the matches, inliers and motions of the oracle and of the
same loop run alone.  The plain family's six small signalled calls (PlainCall, common.h) run in the same rounds on their direct
path -- speculation off, so that none is answered from a frame -- at sizes under the floors of the context's blocks (256 bytes of
scratch, 4096 of pinned memory), then well past 1.5 times the floors, then small again."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import libviso_amd
from libviso_amd import synth
from libviso_amd.abi import MatchParams

import covariance_ref as CR
import disparity_ref as DR
import rectify_ref as RR
import refine_ref as RFR
import sgm_ref as SR
import speckle_ref as K
import subpixel_ref as S
import window_ref as WR
from estimator_util import check_points
from test_gpu_covariance import _check as check_covariance
from test_gpu_disparity import _pair
from test_gpu_drop_in import POSE_TOL, rel_fro
from test_gpu_points import POSE, _param as points_param
from test_gpu_rectify import _hostile_map
from test_gpu_refine import _check as check_refine
from test_speckle_cpu import random_map
from window_cases import check as check_window, direct_frames, hand

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 0)             # small, large, small
SHAPES = ((24, 80), (40, 136))
N_KP, N_MATCH, N_PTS = (8, 40), (5, 30), (6, 30)
BINS = ((16, 2, 2), (40, 4, 2))                 # n_features, nbinx, nbiny: bins of 40 x 12 and 34 x 20 pixels
DISP = dict(num_disp=16, block=5)               # the smallest the parameter checks accept
SPECKLE = dict(max_size=10, max_diff=16)
PLAIN_FRAMES, PLAIN_KP, PLAIN_SEED = 10, 64, 5
SIX_PTS, SIX_MATCH = (6, 3000), (5, 3000)       # the six small plain calls: points of the solver calls, rows of the lists


def _six_inputs(i):
    """The six small plain calls' inputs: keypoints and a match list for collect / triangulate; four lists for match_circle whose
    every second stereo row closes its circle (lr (i, pr[i]), m11 (i, a[i]), lr_prev (j, pp[j]), m22 (k, b[k]): closed when
    pp[a[i]] == b[pr[i]]); a solver case."""
    rng = np.random.default_rng(2000 + i)
    n, nk = SIX_MATCH[i], SIX_MATCH[i] + 3
    kp = [rng.uniform(0, 1000, (nk, 2)).astype(np.float32) for _ in range(2)]
    match = np.stack([rng.integers(0, nk, n), rng.integers(0, nk, n), rng.integers(0, 9999, n)], 1).astype(np.int32)
    pr, a, pp = rng.permutation(n), rng.permutation(n), rng.permutation(n)
    b = np.zeros(n, np.int64)
    b[pr] = (pp[a] + (np.arange(n) % 2)) % n
    rows = lambda q, t: np.stack([q, t, rng.integers(0, 9999, n)], 1).astype(np.int32)   # noqa: E731
    idx = np.arange(n)
    lists = (rows(idx, pr), rows(idx, pp), rows(idx, a), rows(idx, b))   # lr, lr_prev, m11, m22
    X, obs, tr, param = synth.make_solver_case(90 + i, m=SIX_PTS[i], outlier_frac=0.25 * i, noise=0.2)
    return {"kp": kp, "match": match, "lists": lists, "solver": (X, obs, tr, param)}


@functools.lru_cache(maxsize=None)
def inputs(i):
    """Every call's inputs at size i (0 small, 1 large): the same in the child and here."""
    rows, cols = SHAPES[i]
    rng = np.random.default_rng(1000 + i)
    d = {"img": synth.make_images(50 + i, rows, cols)}
    d["kp"] = np.stack([rng.integers(0, cols, N_KP[i]), rng.integers(0, rows, N_KP[i])], 1).astype(np.float32)
    d["kp"][:4] = [[0, 0], [cols - 1, rows - 1], [5, 5], [1, 1]]
    kp2 = np.stack([rng.integers(0, cols, N_KP[i]), rng.integers(0, rows, N_KP[i])], 1).astype(np.float32)
    match = np.stack([rng.integers(0, N_KP[i], N_MATCH[i]), rng.integers(0, N_KP[i], N_MATCH[i]), rng.integers(0, 9999, N_MATCH[i])], 1)
    d["subpixel"] = (d["img"], synth.make_images(60 + i, rows, cols), d["kp"] + np.float32(0.25), kp2, match.astype(np.int32))
    out_shape = (rows - 3, cols - 5)
    d["raw"] = rng.integers(0, 256, (2, rows, cols), dtype=np.uint8)
    d["map"] = _hostile_map(rng, (rows, cols), out_shape) + (out_shape,)
    d["pair"] = _pair(rng, rows, cols)
    d["disp"] = random_map(rng, rows, cols, spread=3, invalid=0.3)
    X, obs, tr, param = synth.make_solver_case(70 + i, m=N_PTS[i], outlier_frac=0.0)
    d["pose"] = (X, obs, tr, np.arange(N_PTS[i], dtype=np.int32), param)
    d["window"] = hand([None] + [[(100 * j + r, 100 * (j - 1) + r) for r in range(N_PTS[i])] for j in (1, 2)])
    d["six"] = _six_inputs(i)
    d["motions"] = np.array([tr] + [tr + rng.normal(0, sd, 6) * np.array([0.05, 0.05, 0.05, 1, 1, 1]) for sd in (1e-4, 1e-2, 0.3) for _ in range(1 + 3 * i)])
    return d


@functools.lru_cache(maxsize=None)
def plain_seq():
    return synth.make_sequence(31, PLAIN_FRAMES, n_kp=PLAIN_KP, width=500, height=200, ragged=True)


# ---- the calls, in the order of their source files ----------------------------------------------------------------------------
def call_extract(i):
    return {"desc": libviso_amd.extract_descriptors(inputs(i)["img"], inputs(i)["kp"])}


def call_harris_response(i):
    return {"resp": libviso_amd.harris_response(inputs(i)["img"])}


def call_detect(i):
    kp, resp = libviso_amd.detect_harris_binned(inputs(i)["img"], *BINS[i])
    return {"kp": kp, "resp": resp}


def call_subpixel(i):
    return {"uv%d" % mode: libviso_amd.refine_stereo_subpixel(*inputs(i)["subpixel"], mode) for mode in (1, 2)}


def call_rectify(i):
    mx, my, out_shape = inputs(i)["map"]
    return {"out": libviso_amd.rectify_images(inputs(i)["raw"], mx, my, out_shape, border=200)}


def call_disparity(i):
    return {"d": libviso_amd.stereo_disparity(*inputs(i)["pair"], **DISP)}


def call_sgm(i):
    return {"d": libviso_amd.stereo_sgm(*inputs(i)["pair"], num_disp=DISP["num_disp"])}


def call_speckle(i):
    return {"d": libviso_amd.filter_speckles(inputs(i)["disp"], **SPECKLE)}


def call_points(i):
    return {"p": libviso_amd.disparity_to_points(inputs(i)["disp"], points_param(), pose=POSE, min_disp16=16)}


def call_covariance(i):
    X, obs, tr, inl, param = inputs(i)["pose"]
    return {"rec": np.asarray(libviso_amd.pose_covariance(X, obs, tr, inl, param, mode=2, sigma=0.3))}


def call_refine(i):
    X, obs, tr, inl, param = inputs(i)["pose"]
    rec, pts = libviso_amd.pose_refine(X, obs, tr, inl, param, mode=1)
    return {"rec": np.asarray(rec), "pts": pts}


def call_window(i):
    frames, param = inputs(i)["window"]
    return {"rec": np.asarray(libviso_amd.window_refine(direct_frames(frames), param, mode=2, sigma=0.3))}


def call_support(i):
    X, obs, _tr, _inl, param = inputs(i)["pose"]
    return {"cnt": libviso_amd.support_sizes(X, obs, inputs(i)["motions"], param)}


def call_six(i):
    from libviso_amd import drop_in
    d = inputs(i)["six"]
    X, obs, tr, param = d["solver"]
    drop_in.plain_speculate(False)   # every call goes to the device
    try:
        x = libviso_amd.collect_matches(d["kp"][0], d["kp"][1], d["match"])
        _, circ, pcl, n = libviso_amd.match_circle(*d["lists"])
        ok, tr_min = libviso_amd.minimize_reproj(X, obs, np.zeros(6), param, np.arange(SIX_PTS[i]))
        inl, rms = libviso_amd.get_inliers(X, obs, tr, param)
        rs_ok, rs_tr, rs_inl = libviso_amd.ransac_minimize_reproj(X, obs, param, seed=4, frame=7 + i)
        return {"x": x, "X": libviso_amd.triangulate_rectified(x, param), "circ": circ, "pcl": pcl, "n": np.int32(n), "ok": np.int32(ok),
                "tr": tr_min, "inl": inl, "rms": np.float64(rms), "rs_ok": np.int32(rs_ok), "rs_tr": rs_tr, "rs_inl": rs_inl}
    finally:
        drop_in.plain_speculate(True)


def call_plain(i, alone=False):
    """The reference's loop body over plain_seq() through the plain family, one call per reference function.  Unless `alone`, the two
    direct calls that share the RANSAC stage's hypothesis slots run between the loop's calls, at size i."""
    seq = plain_seq()
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    out, prev = {}, None

    def between(where):
        if not alone:
            for name, fn in (("detect", call_detect), ("support", call_support)):
                for k, v in fn(i).items():
                    out["%s.%s.%s" % (where, name, k)] = v

    for t in range(PLAIN_FRAMES):
        nL, nR = seq["n"][t]
        kp1, kp2 = seq["kp"][t, 0, :nL].copy(), seq["kp"][t, 1, :nR].copy()
        d1, d2 = seq["desc"][t, 0, :nL].copy(), seq["desc"][t, 1, :nR].copy()
        lr = libviso_amd.match_desc(kp1, kp2, d1, d2, st)
        between("%d.a" % t)
        x = libviso_amd.collect_matches(kp1, kp2, lr)
        X = libviso_amd.triangulate_rectified(x, seq["param"])
        out["%d.lr" % t] = lr
        if prev is not None:
            m11 = libviso_amd.match_desc(kp1, prev["kp1"].copy(), d1, prev["d1"].copy(), tm)
            m22 = libviso_amd.match_desc(kp2, prev["kp2"].copy(), d2, prev["d2"].copy(), tm)
            _, _circ, pcl, n = libviso_amd.match_circle(lr, prev["lr"], m11, m22)
            between("%d.b" % t)
            ok, tr, inl = 0, np.zeros(6), np.zeros(0, np.int32)
            if n >= 3:
                x_c, Xp_c = np.ascontiguousarray(x[:, pcl[:, 0]]), np.ascontiguousarray(prev["X"][:, pcl[:, 1]])
                ok, tr, inl = libviso_amd.ransac_minimize_reproj(Xp_c, x_c, seq["param"], seed=PLAIN_SEED, frame=t)
            out.update({"%d.m11" % t: m11, "%d.m22" % t: m22, "%d.pcl" % t: pcl, "%d.ok" % t: np.int32(ok), "%d.tr" % t: tr,
                        "%d.inl" % t: inl})
        prev = {"kp1": kp1, "kp2": kp2, "d1": d1, "d2": d2, "lr": lr, "X": X}
    return out


ROUND_ROBIN = ("extract", "harris_response", "detect", "subpixel", "rectify", "disparity", "sgm", "speckle", "points", "covariance",
               "refine", "window", "detect", "support", "detect", "plain", "six")
ORDERS = {"round_robin": ROUND_ROBIN, "reverse": ROUND_ROBIN[::-1]}
CALLS = {name[5:]: fn for name, fn in list(globals().items()) if name.startswith("call_")}


def child(order, path):
    from libviso_amd import drop_in
    out = {}
    for p, i in enumerate(SIZES):
        for k, name in enumerate(ORDERS[order]):
            for key, v in CALLS[name](i).items():
                out["%d|%d|%s|%s" % (p, k, name, key)] = v
    served = drop_in.plain_stats()["served"]
    for key, v in call_plain(0, alone=True).items():
        out["alone|%s" % key] = v
    out["served"] = np.asarray(served, np.int64)
    np.savez(path, **out)


# ---- what every call must have returned -----------------------------------------------------------------------------------------
def expect_extract(i, got, oracle):
    assert np.array_equal(got["desc"], oracle.extract_descriptors(inputs(i)["img"], inputs(i)["kp"]))


def expect_harris_response(i, got, oracle):
    assert np.array_equal(got["resp"], oracle.harris_response(inputs(i)["img"]))


@functools.lru_cache(maxsize=None)
def _detect_want(i):
    from oracle import pyoracle
    return pyoracle.detect_harris_binned(inputs(i)["img"], *BINS[i])


def expect_detect(i, got, oracle):
    k0, r0 = _detect_want(i)
    assert len(k0) > 0 and np.array_equal(got["kp"], k0) and np.array_equal(got["resp"], r0)


def expect_subpixel(i, got, oracle):
    for mode in (1, 2):
        want = S.refine(oracle, *inputs(i)["subpixel"], mode)
        assert got["uv%d" % mode].dtype == np.float32 and np.array_equal(got["uv%d" % mode], want), mode


def expect_rectify(i, got, oracle):
    mx, my, _shape = inputs(i)["map"]
    for j, raw in enumerate(inputs(i)["raw"]):
        assert np.array_equal(got["out"][j], RR.remap(raw, mx, my, 200)), j


def expect_disparity(i, got, oracle):
    assert np.array_equal(got["d"], DR.disparity(*inputs(i)["pair"], **DISP))


def expect_sgm(i, got, oracle):
    assert np.array_equal(got["d"], SR.sgm(*inputs(i)["pair"], num_disp=DISP["num_disp"]))


def expect_speckle(i, got, oracle):
    assert np.array_equal(got["d"], K.speckles(inputs(i)["disp"], SPECKLE["max_size"], SPECKLE["max_diff"]))


def expect_points(i, got, oracle):
    assert K.points_equal(got["p"], K.points(inputs(i)["disp"], points_param(), POSE, 16))


def expect_covariance(i, got, oracle):
    X, obs, tr, inl, param = inputs(i)["pose"]
    check_covariance(got["rec"], CR.motion_cov(X, obs, tr, inl, param, 2, 0.3), i)


def expect_refine(i, got, oracle):
    X, obs, tr, inl, param = inputs(i)["pose"]
    want = RFR.refine(X, obs, tr, inl, param, 1, None)
    check_refine(got["rec"], want, i)
    if want["status"] == 1:
        check_points(got["pts"], want, i)


def expect_window(i, got, oracle):
    frames, param = inputs(i)["window"]
    with np.errstate(all="ignore"):
        want = WR.window(frames, len(frames) - 1, len(frames), param, 2, 0.3)
    check_window(got["rec"], want, i)


def expect_support(i, got, oracle):
    X, obs, _tr, _inl, param = inputs(i)["pose"]
    with np.errstate(all="ignore"):
        want = np.array([len(oracle.get_inliers(X, obs, t, param)[0]) for t in inputs(i)["motions"]])
    assert np.array_equal(got["cnt"], want), got["cnt"] - want


def expect_six(i, got, oracle):
    d = inputs(i)["six"]
    X, obs, tr, param = d["solver"]
    x = oracle.collect_matches(d["kp"][0], d["kp"][1], d["match"])
    assert np.array_equal(got["x"], x) and np.array_equal(got["X"], oracle.triangulate_rectified(x, param))
    _, circ, pcl, n = oracle.match_circle(*d["lists"])
    assert n == (SIX_MATCH[i] + 1) // 2 and int(got["n"]) == n and np.array_equal(got["circ"], circ) and np.array_equal(got["pcl"], pcl)
    ok, tr_min, _ = oracle.minimize_reproj(X, obs, np.zeros(6), param, np.arange(SIX_PTS[i]))
    assert int(got["ok"]) == ok
    if ok:
        assert rel_fro(libviso_amd.tr2mat(got["tr"]), oracle.tr2mat(tr_min)) < POSE_TOL
    inl, rms = oracle.get_inliers(X, obs, tr, param)
    assert len(inl) > 0 and np.array_equal(got["inl"], inl) and abs(float(got["rms"]) - rms) <= 1e-12 * max(1, rms)
    rs_ok, rs_tr, rs_inl = oracle.ransac_minimize_reproj(X, obs, param, seed=4, frame=7 + i)
    assert int(got["rs_ok"]) == rs_ok and np.array_equal(got["rs_inl"], rs_inl)
    if rs_ok:
        assert rel_fro(libviso_amd.tr2mat(got["rs_tr"]), oracle.tr2mat(rs_tr)) < POSE_TOL
    if i == 1:
        assert ok and rs_ok and len(rs_inl) > SIX_PTS[i] // 2   # the large case is a real problem, solved


@functools.lru_cache(maxsize=None)
def _plain_want():
    from oracle import pyoracle
    seq = plain_seq()
    st, tm = MatchParams.stereo(seq["F"]), MatchParams.temporal()
    return pyoracle.sequence(seq["kp"], seq["desc"], seq["n"], st, tm, seq["param"], seed=PLAIN_SEED), st, tm


def expect_plain(i, got, oracle, alone=None):
    seq = plain_seq()
    want, st, tm = _plain_want()
    n_ok = 0
    for t in range(PLAIN_FRAMES):
        img = lambda u, side: (seq["kp"][u, side, :seq["n"][u, side]], seq["desc"][u, side, :seq["n"][u, side]])   # noqa: E731
        (kL, dL), (kR, dR) = img(t, 0), img(t, 1)
        assert np.array_equal(got["%d.lr" % t], oracle.match_desc(kL, kR, dL, dR, st)), t
        if t == 0:
            continue
        (pL, pdL), (pR, pdR) = img(t - 1, 0), img(t - 1, 1)
        assert np.array_equal(got["%d.m11" % t], oracle.match_desc(kL, pL, dL, pdL, tm)), t
        assert np.array_equal(got["%d.m22" % t], oracle.match_desc(kR, pR, dR, pdR, tm)), t
        assert int(got["%d.ok" % t]) == want["ok"][t] and len(got["%d.inl" % t]) == want["n_inl"][t], t
        if want["ok"][t]:
            n_ok += 1
            assert rel_fro(libviso_amd.tr2mat(got["%d.tr" % t]), oracle.tr2mat(want["tr"][t])) < POSE_TOL, t
        if alone is not None:   # the same loop with no direct call between its calls
            for k in ("lr", "m11", "m22", "pcl", "ok", "inl"):
                assert np.array_equal(got["%d.%s" % (t, k)], alone["%d.%s" % (t, k)]), (t, k)
            if want["ok"][t]:
                assert rel_fro(libviso_amd.tr2mat(got["%d.tr" % t]), libviso_amd.tr2mat(alone["%d.tr" % t])) < POSE_TOL, t
    assert n_ok >= PLAIN_FRAMES - 3
    for key in got:             # the direct calls between the loop's calls
        parts = key.split(".")
        if len(parts) == 4 and parts[3] in ("kp", "cnt"):
            sub = {k.split(".")[3]: v for k, v in got.items() if k.startswith(".".join(parts[:3]) + ".")}
            EXPECT[parts[2]](i, sub, oracle)


EXPECT = {name[7:]: fn for name, fn in list(globals().items()) if name.startswith("expect_")}


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_any_order_of_direct_calls_gives_every_call_its_answer(viso, oracle, order, tmp_path):
    path = str(tmp_path / "got.npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), order, path]
    r = subprocess.run(cmd, cwd=ROOT, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(path)
    groups = {}
    for key in z.files:
        head, _, leaf = key.rpartition("|")
        groups.setdefault(head, {})[leaf] = z[key]
    alone = groups.pop("alone")
    served = groups.pop("")["served"]
    print("served ahead by the stereo call's frame (match_desc, collect / triangulate, match_circle, ransac):", served.tolist())
    assert served[3] > 0, "no RANSAC stage was running ahead while its slots were borrowed"
    assert len(groups) == len(SIZES) * len(ROUND_ROBIN)
    for head, got in groups.items():
        p, _k, name = head.split("|")
        i = SIZES[int(p)]
        if name == "plain":
            expect_plain(i, got, oracle, alone)
        else:
            EXPECT[name](i, got, oracle)
    expect_plain(0, alone, oracle)


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
