"""numpy restatement of the opt-in sub-pixel stereo refinement (include/viso_hip.h, viso_batch_set_subpixel;
DESIGN.md "Sub-pixel stereo refinement"), built on the oracle's descriptor extractor, plus the CPU assembly of the
image-in pipeline with refined right-image coordinates.  Test infrastructure only.

For a stereo row (i1, i2, dist): p = round(kp1[i1]), q = round(kp2[i2]) (cvRound, half to even);
S_x(d) = SAD(W_L(p), W_R(q.x + d, q.y)), S_y(d) = SAD(W_L(p), W_R(q.x, q.y + d)), d in {-1, 0, 1}, where a window is
MyFeatureExtractor's 11x11 Sobel-x window at that keypoint (oracle_extract_descriptors);
off(S-, S0, S+) = (S- - S+) / (2 (S- + S+ - 2 S0)) in double when S0 <= S-, S0 <= S+ and the denominator is > 0,
else 0; uR' = (float)(q.x + off(S_x)), vR' = (float)(q.y + off(S_y)) in mode 2, (float)q.y in mode 1.
"""
import numpy as np


def parabola_offset(sm, s0, sp):
    """off(S-, S0, S+) on int arrays -> float64 array."""
    sm, s0, sp = (np.asarray(a, np.int64) for a in (sm, s0, sp))
    den = sm + sp - 2 * s0
    ok = (s0 <= sm) & (s0 <= sp) & (den > 0)
    out = np.zeros(np.broadcast(sm, s0, sp).shape, np.float64)
    out[ok] = (sm - sp)[ok].astype(np.float64) / (2.0 * den[ok].astype(np.float64))
    return out


def costs(oracle, imgL, imgR, kp1, kp2, match):
    """(Sx [n][3], Sy [n][3]) int64, columns d = -1, 0, +1."""
    match = np.asarray(match, np.int32).reshape(-1, 3)
    n = len(match)
    if n == 0:
        return np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64)
    kp1 = np.asarray(kp1, np.float32).reshape(-1, 2)
    kp2 = np.asarray(kp2, np.float32).reshape(-1, 2)
    p = np.rint(kp1[match[:, 0]]).astype(np.float32)     # np.rint on float32: half to even, like cvRound / lrintf
    q = np.rint(kp2[match[:, 1]]).astype(np.float32)
    wl = oracle.extract_descriptors(imgL, p).astype(np.int64)
    Sx = np.empty((n, 3), np.int64)
    Sy = np.empty((n, 3), np.int64)
    for c, d in enumerate((-1, 0, 1)):
        qx = q.copy(); qx[:, 0] += d
        qy = q.copy(); qy[:, 1] += d
        Sx[:, c] = np.abs(wl - oracle.extract_descriptors(imgR, qx).astype(np.int64)).sum(1)
        Sy[:, c] = np.abs(wl - oracle.extract_descriptors(imgR, qy).astype(np.int64)).sum(1)
    return Sx, Sy


def refine(oracle, imgL, imgR, kp1, kp2, match, mode=1):
    """viso_refine_stereo_subpixel restated: (n, 2) float32 (uR', vR') per row of `match`."""
    match = np.asarray(match, np.int32).reshape(-1, 3)
    Sx, Sy = costs(oracle, imgL, imgR, kp1, kp2, match)
    q = np.rint(np.asarray(kp2, np.float32).reshape(-1, 2)[match[:, 1]]).astype(np.float64)
    uv = np.empty((len(match), 2), np.float32)
    uv[:, 0] = (q[:, 0] + parabola_offset(Sx[:, 0], Sx[:, 1], Sx[:, 2])).astype(np.float32)
    if mode == 2:
        uv[:, 1] = (q[:, 1] + parabola_offset(Sy[:, 0], Sy[:, 1], Sy[:, 2])).astype(np.float32)
    else:
        uv[:, 1] = (q[:, 1] + 0.0).astype(np.float32)    # q is an integer: a keypoint in [-0.5, -0] gives +0, never -0
    return uv


def extract_all(oracle, seq):
    nf, _, cap, _ = seq["kp"].shape
    desc = np.zeros((nf, 2, cap, 121), np.float32)
    for t in range(nf):
        for side in range(2):
            k = seq["n"][t, side]
            desc[t, side, :k] = oracle.extract_descriptors(seq["images"][t, side], seq["kp"][t, side, :k])
    return desc


def pipeline(oracle, seq, mode, seed=0, first_frame=0, desc=None, stereo=None, temporal=None):
    """The image-in batch path assembled from the oracle's functions, with the stereo observations refined when
    mode != 0: collect_matches -> rows 2-3 replaced by the refined (uR', vR') -> triangulate_rectified / match_circle /
    the gather of src/viso.cpp:1292-1305 -> ransac_minimize_reproj keyed (seed, first_frame + t).
    Returns dict(tr [nf][6], ok, n_inl, lr [nf] stereo lists, uv [nf] refined coordinates (None in mode 0))."""
    from libviso_amd.abi import MatchParams
    st = stereo or MatchParams.stereo(seq["F"])
    tm = temporal or MatchParams.temporal()
    param = seq["param"]
    kp, n, images = seq["kp"], seq["n"], seq["images"]
    nf = kp.shape[0]
    if desc is None:
        desc = extract_all(oracle, seq)
    K = lambda t, s: kp[t, s, :n[t, s]]          # noqa: E731
    D = lambda t, s: desc[t, s, :n[t, s]]        # noqa: E731
    lr, uv, x, X = [], [], [], []
    for t in range(nf):
        m = oracle.match_desc(K(t, 0), K(t, 1), D(t, 0), D(t, 1), st)
        xt = oracle.collect_matches(K(t, 0), K(t, 1), m)
        u = None
        if mode:
            u = refine(oracle, images[t, 0], images[t, 1], K(t, 0), K(t, 1), m, mode)
            xt[2] = u[:, 0].astype(np.float64)
            xt[3] = u[:, 1].astype(np.float64)
        lr.append(m); uv.append(u); x.append(xt); X.append(oracle.triangulate_rectified(xt, param))
    tr = np.zeros((nf, 6)); ok = np.zeros(nf, np.int32); n_inl = np.zeros(nf, np.int32)
    for t in range(1, nf):
        m11 = oracle.match_desc(K(t, 0), K(t - 1, 0), D(t, 0), D(t - 1, 0), tm)
        m22 = oracle.match_desc(K(t, 1), K(t - 1, 1), D(t, 1), D(t - 1, 1), tm)
        r, circ, pcl, cnt = oracle.match_circle(lr[t], lr[t - 1], m11, m22)
        assert r >= 0 and cnt == len(pcl)
        if len(pcl) < 3:
            continue
        x_c = np.ascontiguousarray(x[t][:, pcl[:, 0]])
        Xp_c = np.ascontiguousarray(X[t - 1][:, pcl[:, 1]])
        okt, trt, inl = oracle.ransac_minimize_reproj(Xp_c, x_c, param, seed=seed, frame=first_frame + t)
        tr[t], ok[t], n_inl[t] = trt, okt, len(inl)
    return dict(tr=tr, ok=ok, n_inl=n_inl, lr=lr, uv=uv)


def translation_errors(tr, tr_gt):
    """|t - t_gt| per frame pair 1.. (metres)."""
    return np.linalg.norm(np.asarray(tr)[1:, 3:] - np.asarray(tr_gt)[1:, 3:], axis=1)
