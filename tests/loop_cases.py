"""The loop-closure test scene: 52 stereo frames that drive down one corridor of landmarks, then down a second one that shares
nothing with it, then down the first again, a little to the side and ahead.  Descriptor-only, like libviso_amd.synth: every landmark
carries a base descriptor, every view adds noise; a quarter of every image's keypoints are unrelated clutter.

    frames  0..19   corridor A (x around 0),    1 m a frame
    frames 20..31   corridor B (x around 1000), 1 m a frame
    frames 32..51   corridor A again, 0.3 m to the side and 0.37 m ahead of frames 0..19: frame t's partner is frame t - 32
"""
import numpy as np

from libviso_amd import hostmath, synth
from libviso_amd.abi import DESC_LEN, Param

WIDTH, HEIGHT = 640, 240
F, BASE, CU, CV = synth.KITTI_F, synth.KITTI_BASE, WIDTH / 2.0, HEIGHT / 2.0
N_FRAMES, REVISIT0, JUMPS = 52, 32, (20, 32)     # JUMPS: the frames whose predecessor is somewhere else
PER_METRE, LENGTH, HALF_X, HALF_Y = 40, 90.0, 12.0, 3.0
Z_NEAR, Z_FAR = 4.0, 60.0
P1 = np.array([[F, 0, CU, 0], [0, F, CV, 0], [0, 0, 1, 0]], np.float64)
P2 = np.array([[F, 0, CU, -F * BASE], [0, F, CV, 0], [0, 0, 1, 0]], np.float64)


def corridor_of(t):
    return 1 if 20 <= t < 32 else 0


def partner_of(t):
    """The frame of the first pass that frame t (32..51) is nearest to."""
    return t - REVISIT0


def _hash(idx):
    """A fixed 32-bit hash of the landmark index (the same on every visit)."""
    x = (np.asarray(idx, np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    return (x >> np.uint64(32)).astype(np.int64)


def true_poses(rng):
    """[52][4][4] camera to world."""
    poses = np.zeros((N_FRAMES, 4, 4))
    for t in range(N_FRAMES):
        if t < 20:
            c = np.array([0.0, 0.0, float(t)])
        elif t < 32:
            c = np.array([1000.0, 0.0, float(t - 20)])
        else:
            c = np.array([0.3, 0.0, (t - REVISIT0) + 0.37])
        R = synth.rot_from_tr(np.concatenate([rng.uniform(-0.02, 0.02, 3), np.zeros(3)]))[0]
        poses[t, :3, :3], poses[t, :3, 3], poses[t, 3, 3] = R, c, 1.0
    return poses


def make_case(seed, n_kp=256):
    """dict(kp f32 [52][2][cap][2], desc int16 [52][2][cap][121], n [52][2], poses, param, F, stereo: per frame the true stereo list
    [m][3] (left index, right index, 0) of the landmarks both images hold)."""
    rng = np.random.default_rng(seed)
    n_lm = int(PER_METRE * LENGTH)
    world, base = [], []
    for x0 in (0.0, 1000.0):
        world.append(np.stack([x0 + rng.uniform(-HALF_X, HALF_X, n_lm), rng.uniform(-HALF_Y, HALF_Y, n_lm), rng.uniform(0.0, LENGTH, n_lm)], 1))
        base.append(synth._new_desc(rng, n_lm))
    order = np.argsort(_hash(np.arange(n_lm)), kind="stable")
    poses = true_poses(rng)
    n_in = int(round(0.75 * n_kp))
    kp = np.zeros((N_FRAMES, 2, n_kp, 2), np.float32)
    desc = np.zeros((N_FRAMES, 2, n_kp, DESC_LEN), np.int16)
    n = np.full((N_FRAMES, 2), n_kp, np.int32)
    stereo = []
    for t in range(N_FRAMES):
        W, D = world[corridor_of(t)], base[corridor_of(t)]
        Xc = (W - poses[t, :3, 3]) @ poses[t, :3, :3]          # R' (X - c)
        uL, v, uR = F * Xc[:, 0] / Xc[:, 2] + CU, F * Xc[:, 1] / Xc[:, 2] + CV, F * (Xc[:, 0] - BASE) / Xc[:, 2] + CU
        with np.errstate(invalid="ignore"):
            vis = (Xc[:, 2] >= Z_NEAR) & (Xc[:, 2] <= Z_FAR) & (uL >= 0) & (uL <= WIDTH - 1) & (uR >= 0) & (uR <= WIDTH - 1) & (v >= 0) & (v <= HEIGHT - 1)
        pick = order[vis[order]][:n_in]                          # the visible landmarks in hash order
        assert len(pick) == n_in, (t, len(pick))
        where = []
        for side, u in ((0, uL), (1, uR)):
            xy = np.empty((n_kp, 2))
            xy[:n_in] = np.stack([u[pick], v[pick]], 1) + rng.normal(0.0, 0.3, (n_in, 2))
            xy[n_in:] = np.stack([rng.uniform(0, WIDTH - 1, n_kp - n_in), rng.uniform(0, HEIGHT - 1, n_kp - n_in)], 1)
            dd = np.empty((n_kp, DESC_LEN), np.int16)
            dd[:n_in] = np.clip(D[pick] + np.rint(rng.normal(0.0, 6.0, (n_in, DESC_LEN))), -1020, 1020)
            dd[n_in:] = synth._new_desc(rng, n_kp - n_in)
            perm = rng.permutation(n_kp)
            kp[t, side], desc[t, side] = xy[perm], dd[perm]
            inv = np.empty(n_kp, np.int64)
            inv[perm] = np.arange(n_kp)
            where.append(inv[:n_in])
        st = np.stack([where[0], where[1], np.zeros(n_in, np.int64)], 1).astype(np.int32)
        stereo.append(st[np.argsort(st[:, 0])])
    param = Param.default(base=BASE, f=F, cu=CU, cv=CV)
    return dict(kp=kp, desc=desc, n=n, poses=poses, param=param, F=hostmath.F_from_P(P1, P2), stereo=stereo, n_kp=n_kp)


def relative(poses, i, j):
    """P_i^-1 P_j: what an edge (i, j) measures."""
    return np.linalg.inv(poses[i]) @ poses[j]


def near_partner(i, j):
    return j >= REVISIT0 and abs(i - partner_of(j)) <= 4


def check_edges(case, edges, z_tol_near, z_tol_other):
    """The three assertions of the purpose, on edges [(frame_i, frame_j, Z, ...)]: every revisit frame has an edge to a frame within 4
    of its partner, no edge joins the corridors, every Z is the true relative pose -- within z_tol_near for those edges, z_tol_other
    for any other.  Returns the worst |Z - truth| of either kind."""
    worst = [0.0, 0.0]
    for e in edges:
        i, j, Z = int(e[0]), int(e[1]), e[2]
        assert i < j and corridor_of(i) == corridor_of(j), (i, j)
        err, other = np.abs(Z - relative(case["poses"], i, j)).max(), not near_partner(i, j)
        worst[other] = max(worst[other], err)
        assert err <= (z_tol_other if other else z_tol_near), (i, j, err)
    for t in range(REVISIT0, N_FRAMES):
        assert any(int(e[1]) == t and near_partner(int(e[0]), t) for e in edges), t
    return worst
