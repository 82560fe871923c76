"""bench.py's own launch shapes against the oracle: 513 frames (512 pairs) x 2000 keypoints, several batches in flight
on several contexts, round robin without a sync, plus the int16, whole-pipeline, streaming, clustered, image-in,
device-Harris, configs[4] and drop-in legs at the sizes bench.py runs them.

Only at this size do the last 8-frame problem group (prob_slot: one real frame and 23 empty slots), block indices past
16 k, RANSAC keys past 512, the learnt 8-bit plane shift and a loaded overflow queue appear.  Every comparison is exact
(lists, counters, ok, n_inl) or the 1e-5 pose bound of test_config2_3_full_size_vs_oracle; the oracle runs in chunks
on a thread pool (tests/bench_oracle.py, proven equal to one whole call by tests/test_bench_oracle_cpu.py).
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import libviso_amd
from libviso_amd import drop_in, synth
from libviso_amd.abi import MatchParams

import bench_oracle as bo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF = 513                      # bench.py --frames 512: 512 pairs + the one-frame halo
KP = 2000
T = (0, 1, 2, 7, 8, 9, 255, 256, 257, 504, 505, 511, 512)     # the 8-frame group boundaries, first and last groups
KINDS = (0, 1, 2)
# overflow_count() of one whole-pipeline step on the clustered bench sequence (--clustered 0.7), measured on an MI355X:
# 9103..9112 on three lanes over two runs (the 8-bit plane shift learnt: 3)
CLUSTERED_OVERFLOW_MEASURED = 9100


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    print(f"\n[{request.node.name}: {time.perf_counter() - t0:.1f} s]", flush=True)


def _params(seq):
    return MatchParams.stereo(seq["F"]), MatchParams.temporal()


def _lane(seq, nf=NF, cap=KP, first_frame=0, upload=True):
    c = libviso_amd.Context(0)
    libviso_amd.set_matcher_variant(libviso_amd.DEFAULT_MATCHER, c)
    b = libviso_amd.Batch(c, nf, cap)
    if upload:
        b.upload(seq["kp"], seq["desc"], seq["n"])
    st, tm = _params(seq)
    b.set_params(st, tm, seq["param"], seed=1, first_frame=first_frame)
    return c, b


def _close(lanes):
    for c, b in lanes:
        b.close()
        c.close()


def _round_robin(lanes, fn, calls):
    for i in range(calls):
        fn(lanes[i % len(lanes)][1])
    for c, _ in lanes:
        c.synchronize()


def check_counters(b, want, tag, frames=None):
    sc, mo = b.counters()
    if frames is not None:
        sc, mo = sc[:, frames], mo[:, frames]
    for name, got, w in (("scored", sc, want["scored"]), ("m_out", mo, want["m_out"])):
        bad = np.flatnonzero((got != w).any(0))
        assert bad.size == 0, (tag, name, "frames", bad[:8], got[:, bad[:4]], w[:, bad[:4]])


def check_lists(b, wl, tag, frame_of=lambda t: t):
    for (w, t), (m, _) in wl.items():
        got = b.matches(w, frame_of(t))
        assert np.array_equal(got, m), (tag, "kind", w, "frame", frame_of(t), len(got), len(m))


def check_poses(tr, ok, n_inl, want, tag, frames):
    assert np.array_equal(ok, want["ok"]), (tag, "ok differs at", frames[np.flatnonzero(ok != want["ok"])][:8])
    assert np.array_equal(n_inl, want["n_inl"]), (tag, "n_inl differs at", frames[np.flatnonzero(n_inl != want["n_inl"])][:8])
    for i, t in enumerate(frames):
        a, r = libviso_amd.tr2mat(tr[i]), bo.oracle.tr2mat(want["tr"][i])
        assert np.linalg.norm(a - r) / np.linalg.norm(r) < 1e-5, (tag, "tr at frame", t, tr[i], want["tr"][i])


def check_batch(b, want, wl, tag):
    """Counters and poses over every frame, lists at the frames of wl."""
    check_counters(b, want, tag)
    check_lists(b, wl, tag)
    tr, ok, n_inl = b.poses()
    check_poses(tr, ok, n_inl, want, tag, np.arange(len(ok)))


def _reversed(seq):
    r = dict(seq)
    for k in ("kp", "desc", "n"):
        r[k] = np.ascontiguousarray(seq[k][::-1])
    return r


# ---------------------------------------------------------------------------------------------------------------------
# the bench sequence: bench.py's make_sequence(1000 + rank, 513, n_kp=2000), seed 1, first_frame 0

class TestBenchSequence:
    @pytest.fixture(scope="class")
    def bench(self, oracle):
        t0 = time.perf_counter()
        seq = synth.make_sequence(1000, NF, n_kp=KP)
        st, tm = _params(seq)
        want = bo.sequence_chunked(seq["kp"], seq["desc"], seq["n"], st, tm, seq["param"], seed=1)
        assert want["ok"][1:].mean() > 0.95
        d = {"seq": seq, "want": want, "lists": bo.lists(seq, T, KINDS, st, tm), "memo": {}}
        print(f"\n[bench sequence + oracle: {time.perf_counter() - t0:.1f} s]", flush=True)
        yield d
        d.clear()

    def test_a_headline_dump_equals_oracle(self, bench, tmp_path):
        """bench.py's plain run (the headline alone) with --dump-outputs: every frame's three lists of the dumped step."""
        out = tmp_path / "dump"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--dump-outputs", str(out)],
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        print(r.stdout.strip().splitlines()[-1][:300])
        frames = np.load(out / "frames.npy").astype(np.int64)
        assert np.array_equal(frames, np.arange(NF))            # ~35 MB: under the 64 MB cap, nothing sampled
        seq = bench["seq"]
        st, tm = _params(seq)
        wl = bo.lists(seq, range(NF), KINDS, st, tm)
        for w, kind in enumerate(("stereo", "temporal_left", "temporal_right")):
            m = np.load(out / f"{kind}_matches.npy").astype(np.int64)
            cnt = np.load(out / f"{kind}_counts.npy").astype(np.int64)
            assert len(cnt) == NF and cnt.sum() == len(m)
            per = np.split(m, np.cumsum(cnt)[:-1])
            for t in range(NF):
                got = per[t]
                want = wl[(w, t)][0] if (w == 0 or t >= 1) else np.zeros((0, 3), np.int32)
                assert np.all(got[:, 0] == t), (kind, t)
                assert np.array_equal(got[:, 1:], want), (kind, "frame", t, len(got), len(want))

    def test_b_three_lanes_matcher_only(self, bench):
        """bench.py's headline lanes: 3 contexts, run_matcher round robin without a sync, the 8-bit plane shift learnt
        from the counting runs (the first and every VISO_R8_EVERY-th run) whose counts come back asynchronously."""
        seq, want = bench["seq"], bench["want"]
        lanes = [_lane(seq) for _ in range(3)]
        try:
            _round_robin(lanes, lambda b: b.run_matcher(), 60)     # 20 runs per lane: two counting runs each
            _round_robin(lanes, lambda b: b.run_matcher(), 3)      # one more each, after every count has come back
            for i, (_, b) in enumerate(lanes):
                print(f"lane {i}: row8_shift {b.row8_shift()}")
                check_counters(b, want, f"lane {i}")
                check_lists(b, bench["lists"], f"lane {i}")
            bench["memo"]["b_lists"] = {k: lanes[0][1].matches(*k) for k in bench["lists"]}
            bench["memo"]["b_counters"] = lanes[0][1].counters()
        finally:
            _close(lanes)

    def test_c_int16_rows(self, bench):
        """bench.py's resident_i16 leg: the same step from desc.astype(np.int16) rows, synchronous and asynchronous."""
        seq, want = bench["seq"], bench["want"]
        d16 = np.ascontiguousarray(seq["desc"].astype(np.int16))
        lanes = [_lane(seq, upload=False) for _ in range(3)]
        pk = pd = None
        try:
            for _, b in lanes:
                b.upload_i16(seq["kp"], d16, seq["n"])
            _round_robin(lanes, lambda b: b.run_matcher(), 51)
            for i, (_, b) in enumerate(lanes):
                check_counters(b, want, f"i16 lane {i}")
                check_lists(b, bench["lists"], f"i16 lane {i}")
                if "b_counters" in bench["memo"]:
                    sc, mo = b.counters()
                    assert np.array_equal(sc, bench["memo"]["b_counters"][0]) and np.array_equal(mo, bench["memo"]["b_counters"][1])
                    assert all(np.array_equal(b.matches(*k), m) for k, m in bench["memo"]["b_lists"].items())
            pk = libviso_amd.PinnedArray(seq["kp"].shape, np.float32)
            pd = libviso_amd.PinnedArray(d16.shape, np.int16)
            pk.a[...] = seq["kp"]
            pd.a[...] = d16
            c, b = lanes[0]
            b.upload_i16(pk.a, pd.a, seq["n"], asynchronous=True)
            b.run_matcher()
            c.synchronize()
            check_counters(b, want, "i16 async")
            check_lists(b, bench["lists"], "i16 async")
        finally:
            _close(lanes)
            for p in (pk, pd):
                if p is not None:
                    p.close()

    def test_d_whole_pipeline_five_lanes(self, bench, oracle):
        """bench.py's whole-pipeline legs (--e2e-streams 5): run() round robin, twice per lane; a sixth lane keyed as rank 1
        of --gpus 2 (first_frame 512: RANSAC keys 512..1024)."""
        seq, want = bench["seq"], bench["want"]
        lanes = [_lane(seq) for _ in range(5)]
        try:
            _round_robin(lanes, lambda b: b.run(), 10)
            for i, (_, b) in enumerate(lanes):
                check_batch(b, want, bench["lists"], f"e2e lane {i}")
                for t in T[1:]:
                    circ, pcl = b.circle(t)
                    _, wc, wp, _ = oracle.match_circle(b.matches(0, t), b.matches(0, t - 1), b.matches(1, t), b.matches(2, t))
                    assert len(circ) > 100 and np.array_equal(circ, wc) and np.array_equal(pcl, wp), (i, t)
            bench["memo"]["d_lists"] = {k: lanes[0][1].matches(*k) for k in bench["lists"]}
        finally:
            _close(lanes)
        st, tm = _params(seq)
        want512 = bo.sequence_chunked(seq["kp"], seq["desc"], seq["n"], st, tm, seq["param"], seed=1, first_frame=512)
        assert not np.array_equal(want512["tr"], want["tr"])
        lane = [_lane(seq, first_frame=512)]
        try:
            _round_robin(lane, lambda b: b.run(), 2)
            check_batch(lane[0][1], want512, bench["lists"], "first_frame 512")
        finally:
            _close(lane)

    def test_e_streaming_alternation(self, bench):
        """bench.py's streaming legs: one resident batch fed forward, time-reversed, forward from pinned memory; every run
        must equal the oracle of the order just uploaded (no sort, shift, flag or family state left from the last)."""
        seq, want = bench["seq"], bench["want"]
        rseq = _reversed(seq)
        st, tm = _params(seq)
        rwant = bo.sequence_chunked(rseq["kp"], rseq["desc"], rseq["n"], st, tm, seq["param"], seed=1)
        rl = bo.lists(rseq, T, KINDS, st, tm)
        hosts, h16 = [], []
        lane = [_lane(seq, upload=False)]
        c, b = lane[0]
        try:
            for s in (seq, rseq):
                pk = libviso_amd.PinnedArray(s["kp"].shape, np.float32)
                pd = libviso_amd.PinnedArray(s["desc"].shape, np.float32)
                pk.a[...] = s["kp"]
                pd.a[...] = s["desc"]
                hosts.append((pk, pd, s["n"]))
            orders = ((0, want, bench["lists"]), (1, rwant, rl), (0, want, bench["lists"]))
            for i, w, wl in orders:
                pk, pd, nn = hosts[i]
                b.upload_async(pk.a, pd.a, nn)
                b.run()
                c.synchronize()
                check_batch(b, w, wl, f"stream f32 {'reversed' if i else 'forward'}")
            for pk, pd, _ in hosts:
                pd.close()
            for s in (seq, rseq):
                p = libviso_amd.PinnedArray(s["desc"].shape, np.int16)
                p.a[...] = s["desc"].astype(np.int16)
                h16.append(p)
            for i, w, wl in orders[1:]:
                pk, _, nn = hosts[i]
                b.upload_i16(pk.a, h16[i].a, nn, asynchronous=True)
                b.run()
                c.synchronize()
                check_batch(b, w, wl, f"stream i16 {'reversed' if i else 'forward'}")
        finally:
            _close(lane)
            for pk, pd, _ in hosts:
                pk.close()
                pd.close()
            for p in h16:
                p.close()

    def test_i_drop_in_loop(self, bench):
        """bench.py's drop_in_per_call leg: the plain per-call C-ABI over the first 257 frames, with the image cache and
        speculation on, and with every call direct."""
        seq, want = bench["seq"], bench["want"]
        nd = 257
        dk, dd, dn = seq["kp"][:nd], seq["desc"][:nd], seq["n"][:nd]
        wd = {k: want[k][:nd] for k in ("tr", "ok", "n_inl")}
        try:
            for speculate in (True, False):
                drop_in.plain_cache(True)
                drop_in.plain_speculate(speculate)
                drop_in.run(dk[:12], dd[:12], dn[:12], seq["F"], seq["param"], seed=1)
                o = drop_in.run(dk, dd, dn, seq["F"], seq["param"], seed=1, want_matches=True)
                tag = f"drop-in speculate={speculate}"
                check_poses(o["tr"], o["ok"], o["n_inl"], wd, tag, np.arange(nd))
                for (w, t), (m, _) in bench["lists"].items():
                    if t < nd:
                        assert np.array_equal(o["matches"][w][t], m), (tag, w, t)
                        if "d_lists" in bench["memo"]:
                            assert np.array_equal(o["matches"][w][t], bench["memo"]["d_lists"][(w, t)])
        finally:
            drop_in.plain_cache(True)
            drop_in.plain_speculate(True)


# ---------------------------------------------------------------------------------------------------------------------
# image-in legs: make_image_sequence(2000 + rank, 513, n_kp=2000)

def _slice_check(b, kp, desc, n, seq, t, tag, oracle):
    """Frame t of batch b against the oracle over the two-frame slice [t - 1, t] (RANSAC key t - 1 + 1 = t)."""
    lo = max(0, t - 1)
    st, tm = _params(seq)
    w = oracle.sequence(kp[lo:t + 1], desc[lo:t + 1], n[lo:t + 1], st, tm, seq["param"], seed=1, first_frame=lo)
    k = t - lo
    mini = {"kp": kp[lo:t + 1], "desc": desc[lo:t + 1], "n": n[lo:t + 1]}
    wl = bo.lists(mini, [k], KINDS, st, tm, workers=3)
    check_lists(b, wl, tag, frame_of=lambda j: lo + j)
    check_counters(b, {"scored": w["scored"][:, k:k + 1], "m_out": w["m_out"][:, k:k + 1]}, (tag, t), frames=[t])
    tr, ok, n_inl = b.poses()
    check_poses(tr[t:t + 1], ok[t:t + 1], n_inl[t:t + 1],
                {"tr": w["tr"][k:k + 1], "ok": w["ok"][k:k + 1], "n_inl": w["n_inl"][k:k + 1]}, tag, np.array([t]))
    return w["ok"][k]


def _frames_with_halo(frames):
    return sorted({f for t in frames for f in (t - 1, t) if f >= 0})


class TestImageSequence:
    @pytest.fixture(scope="class")
    def iseq(self):
        t0 = time.perf_counter()
        d = {"seq": synth.make_image_sequence(2000, NF, n_kp=KP)}
        print(f"\n[image sequence: {time.perf_counter() - t0:.1f} s]", flush=True)
        yield d
        d.clear()

    def _desc(self, oracle, images, kp, n, frames):
        desc = np.zeros(kp.shape[:3] + (121,), np.float32)
        for t in frames:
            for s in range(2):
                desc[t, s, :n[t, s]] = oracle.extract_descriptors(images[t, s], kp[t, s, :n[t, s]])
        return desc

    def test_g_image_in_five_lanes(self, iseq, oracle):
        seq = iseq["seq"]
        lanes = [_lane(seq, upload=False) for _ in range(5)]
        try:
            for _, b in lanes:
                b.upload_images(seq["images"], seq["kp"], seq["n"])
            _round_robin(lanes, lambda b: b.run_images(False), 10)
            desc = self._desc(oracle, seq["images"], seq["kp"], seq["n"], _frames_with_halo(T))
            for i, (_, b) in enumerate(lanes):
                oks = [_slice_check(b, seq["kp"], desc, seq["n"], seq, t, f"image lane {i}", oracle) for t in T]
                assert sum(oks) >= len(T) - 2
        finally:
            _close(lanes)

    def test_g_device_harris(self, iseq, oracle):
        seq = iseq["seq"]
        cap = 1200
        lane = [_lane(seq, cap=cap, upload=False)]
        c, b = lane[0]
        try:
            b.upload_images_only(seq["images"])
            for _ in range(2):
                b.detect()
                b.run_images(False)
            c.synchronize()
            fr = _frames_with_halo(T)
            kp = np.zeros((NF, 2, cap, 2), np.float32)
            n = np.zeros((NF, 2), np.int32)
            for t in fr:
                for s in range(2):
                    k, _ = oracle.detect_harris_binned(seq["images"][t, s])
                    kp[t, s, :len(k)], n[t, s] = k, len(k)
                    assert np.array_equal(b.keypoints(t, s), k), ("harris", t, s)
            desc = self._desc(oracle, seq["images"], kp, n, fr)
            oks = [_slice_check(b, kp, desc, n, seq, t, "device harris", oracle) for t in T]
            assert sum(oks) >= len(T) - 2
        finally:
            _close(lane)


# ---------------------------------------------------------------------------------------------------------------------

def test_f_clustered(viso, oracle):
    """bench.py --clustered 0.7: ~70 % of the features in blobs, thousands of queries per step through the overflow
    kernel (K cap, exact SAD ties, LDS list overflow)."""
    seq = synth.make_sequence(1000, NF, n_kp=KP, cluster_frac=0.7)
    st, tm = _params(seq)
    want = bo.sequence_chunked(seq["kp"], seq["desc"], seq["n"], st, tm, seq["param"], seed=1)
    wl = bo.lists(seq, T, KINDS, st, tm)
    lanes = [_lane(seq) for _ in range(3)]
    try:
        _round_robin(lanes, lambda b: b.run(), 6)
        for i, (_, b) in enumerate(lanes):
            nov = b.overflow_count()
            print(f"clustered lane {i}: overflow_count {nov}, row8_shift {b.row8_shift()}")
            assert nov >= CLUSTERED_OVERFLOW_MEASURED // 2
            check_batch(b, want, wl, f"clustered lane {i}")
    finally:
        _close(lanes)


def test_h_config5_past_2g_bytes(viso, oracle):
    """configs[4] (2048x1024, 8000 keypoints) at 300 frames: 2.3 GB of f32 descriptors, so the last frames' rows start
    past byte 2^31 of the uploaded matrix.  The device's u16 row matrix stays below 2^31 bytes at this size: crossing it
    there too would take at least 525 pairs at 8000 keypoints, which this test does not cover."""
    nf, kp_n = 300, 8000
    seq = synth.make_sequence(102, nf, n_kp=kp_n, width=2048, height=1024)
    assert seq["desc"][297].nbytes * 297 > 2 ** 31
    lane = [_lane(seq, nf=nf, cap=kp_n)]
    c, b = lane[0]
    try:
        b.run()
        c.synchronize()
        oks = [_slice_check(b, seq["kp"], seq["desc"], seq["n"], seq, t, "configs[4]", oracle) for t in (1, 150, 297, 298, 299)]
        assert all(oks)
    finally:
        _close(lane)
        seq.clear()
