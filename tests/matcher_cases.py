"""Hand-built match_desc problems that sit ON the fixed capacities of the matcher kernels, and the plain model that proves
each one sits where it claims (tests/test_matcher_cases_cpu.py); tests/test_gpu_matcher_capacity.py holds the device to the
oracle on them, bit for bit.  No GPU and no library here: numpy only.

The capacities (checked against the `#define`s of libviso_amd/csrc by the CPU test: a capacity that moves fails there and
the cases below move with it):

  UCAP      union-list entries of a round; one more and the whole round leaves for match_overflow_kernel
  S8ROWS    list positions whose SAD8 byte match_union8_kernel keeps for its rescue; a longer list switches the rescue off
  KPCAP     window keypoints staged in LDS; the tail [KPCAP, W) is scanned from global memory, 32 per step
  NP        passes of 8 rows in flight in the union pipelines (prologue / steady state / epilogue)
  K         max_neighbors: `nu > K` changes how the scored pairs are counted, `c > K` sends the query away
  OVF_STAGE in-radius targets of one query that match_overflow_kernel stages
  ST_WCAP   window keypoints per chunk of match_stereo_kernel, ST_SLOTS candidates per query and pass of its walk
  MB_SEG    pair-list entries per query of match_batch_kernel

How a problem is cut up (the kernels' header comments, restated in `model`):
  * the targets are grouped by a map of NB column buckets over their x range; a tile of up to 64 queries sees the whole
    buckets that cover [min qx - radius, max qx + radius]: W keypoints, in bucket order (no order inside a bucket);
  * a tile's queries are taken in y order, eight per round (wave w, round r: y ranks 16 w + 8 r .. + 7);
  * a round's union list holds every window keypoint within the L1 radius of at least one of its queries: nu entries;
    c = a query's own in-radius count.

Layout rules that keep the model this small: at most 64 queries (one tile) with distinct y; target 0 far outside every radius
(the walk's stop at target index 0, src/viso.cpp:693, cuts nothing); every target's x inside [min qx - radius, max qx + radius],
so W == n2; non-members are far away in y; integer coordinates, members well inside the radius; where members must sit at the
window's end they have a larger x than every filler by many bucket widths (`pos_bounds` proves the positions).

Two descriptor families, for the planes' shift 3 (set_row8_shift(3)):
  clear  values in +-1000; a query has ONE planted best at SAD 10 + i, every other candidate at SAD >= CLEAR_GAP: with
         (SAD8 << 3) >= SAD - 121 * 7 and the bound's slack of 896, L3 >= SAD - 1743 >= 18257 clears both verdict tests of
         match_union8_kernel at ratio 0.9 — no rescue, no hand-over;
  flat   values in 0..7: every plane byte is the same, SAD8 = 0 and L = -896 for every candidate, nothing is ever cleared:
         a query with three or more members needs the rescue (or, where the rescue is off, the overflow kernel).  Queries
         carry the zero descriptor, a target's values sum to its SAD; a query's candidates have pairwise distinct SADs.
"""
import functools

import numpy as np

from libviso_amd.abi import MatchParams

# ---------------------------------------------------------------- the capacities (name here -> (#define, files of csrc))
UCAP, PAD, S8ROWS, KPCAP, NP, G, QPB, NB = 448, 32, 176, 512, 2, 8, 64, 256
OVF_STAGE, ST_WCAP, ST_SLOTS, MB_SEG = 768, 384, 8, 128
CAPACITIES = {
    "UCAP": (UCAP, [("MU_UCAP", "match_union8.hip"), ("MU_UCAP", "match_union.hip"), ("MP_UCAP", "match_prune.hip")], "union_list"),
    "PAD": (PAD, [("MU_PAD", "match_union8.hip"), ("MU_PAD", "match_union.hip")], "union_list"),
    "S8ROWS": (S8ROWS, [("MU_S8ROWS", "match_union8.hip")], "store"),
    "KPCAP": (KPCAP, [("MU_KPCAP", "match_union8.hip"), ("MU_KPCAP", "match_union.hip"), ("MP_KPCAP", "match_prune.hip"),
                      ("MB_KPCAP", "match_batch.hip")], "window"),
    "NP": (NP, [("MU_NP", "match_union8.hip"), ("MU_NP", "match_union.hip")], "pipeline"),
    "G": (G, [("MU_G", "match_union8.hip"), ("MU_G", "match_union.hip"), ("MP_G", "match_prune.hip")], "all (the rounds)"),
    "QPB": (QPB, [("MU_QPB", "match_union8.hip"), ("MU_QPB", "match_union.hip"), ("MP_QPB", "match_prune.hip"),
                  ("MB_QPB", "match_batch.hip"), ("ST_QPW", "match_stereo.hip")], "all (one tile)"),
    "NB": (NB, [("VISO_NB", "common.h")], "all (the window)"),
    "OVF_STAGE": (OVF_STAGE, [("VISO_OVF_STAGE", "match.hip")], "staging"),
    "ST_WCAP": (ST_WCAP, [("ST_WCAP", "match_stereo.hip")], "stereo"),
    "ST_SLOTS": (ST_SLOTS, [("ST_SLOTS", "match_stereo.hip")], "stereo"),
    "MB_SEG": (MB_SEG, [("MB_SEG", "match_batch.hip")], "batch"),
}
R8_SHIFT = 3
CLEAR_GAP = 20000
DLEN = 121
RADIUS = 80
QX, QY = 1000, 1000
FAMILIES = ("clear", "flat")


class Case:
    """One named problem: args() = (kp1, kp2, d1, d2, mp); claims = what the constructor says about it."""

    def __init__(self, name, kp1, kp2, d1, d2, mp, claims):
        self.name, self.kp1, self.kp2, self.d1, self.d2, self.mp, self.claims = name, kp1, kp2, d1, d2, mp, claims

    def args(self):
        return self.kp1, self.kp2, self.d1, self.d2, self.mp

    def __iter__(self):
        return iter((self.kp1, self.kp2, self.d1, self.d2, self.mp, self.claims))

    def __repr__(self):
        return self.name


# ---------------------------------------------------------------- the model
def l1(kp1, kp2):
    """cvflann::L1 of two floats, as the oracle and the kernels add it: |dx| + |dy| in float."""
    a, b = np.asarray(kp1, np.float32), np.asarray(kp2, np.float32)
    return np.abs(a[:, None, 0] - b[None, :, 0]) + np.abs(a[:, None, 1] - b[None, :, 1])


def buckets(kp2):
    """Column bucket of every target (sort_kp_kernel: NB buckets over [min x, max x], the last one closed)."""
    x = np.asarray(kp2, np.float32)[:, 0]
    x0, x1 = x.min(), x.max()
    scale = np.float32(NB) / (x1 - x0) if x1 > x0 else np.float32(0)
    return np.clip(np.floor((x - x0) * scale), 0, NB - 1).astype(int), x0, scale


def window(kp1, kp2, radius):
    """Mask of the targets in the tile's window: the whole buckets that cover [min qx - radius, max qx + radius]."""
    b, x0, scale = buckets(kp2)
    f32 = np.float32
    xa, xb, r = f32(np.min(kp1[:, 0])), f32(np.max(kp1[:, 0])), f32(radius)
    slack = (abs(xa) + abs(xb) + abs(r)) * f32(1e-6) + f32(1e-6)
    bo = lambda x: int(np.clip(np.floor((f32(x) - x0) * scale), 0, NB - 1))   # noqa: E731
    return (b >= bo(xa - r - slack)) & (b <= bo(xb + r + slack))


def rounds_of(kp1):
    """The tile's queries in y order, eight per round.  Up to eight queries are one round whatever their order."""
    y = np.asarray(kp1)[:, 1]
    assert len(y) <= QPB, "one tile"
    assert len(y) <= G or len(set(y.tolist())) == len(y), "distinct y: the y order is the round composition"
    order = np.argsort(y, kind="stable")
    return [order[i:i + G] for i in range(0, len(order), G)]


def model(kp1, kp2, mp):
    """dict(W, nu per round, c per round and query in y order) of a temporal problem."""
    r = np.float32(mp.radius)
    D = l1(kp1, kp2)
    assert (D[:, 0] > r).all(), "target 0 is outside every radius"
    M = D <= r
    win = window(kp1, kp2, mp.radius)
    assert win[M.any(0)].all()
    rounds = rounds_of(kp1)
    return dict(W=int(win.sum()), nu=[int((M[q].any(0) & win).sum()) for q in rounds],
                c=[[int(M[i].sum()) for i in q] for q in rounds])


def model_stereo(kp1, kp2, mp):
    """dict(W, c per query, row = in-radius targets on the query's own row: they pass the gate of a rectified pair)."""
    r = np.float32(mp.radius)
    D = l1(kp1, kp2)
    assert (D[:, 0] > r).all()
    M = D <= r
    win = window(kp1, kp2, mp.radius)
    assert win[M.any(0)].all() and len(kp1) <= QPB
    same = np.asarray(kp1)[:, None, 1] == np.asarray(kp2)[None, :, 1]
    return dict(W=int(win.sum()), c=[int(v) for v in M.sum(1)], row=[int(v) for v in (M & same).sum(1)])


def pos_bounds(kp1, kp2, radius, group):
    """(first, last) window position a target of `group` can have: the order inside a bucket is not defined, the order of the
    buckets is.  The group's buckets are its own, at least `gap` empty buckets away from everybody else's."""
    b, _, _ = buckets(kp2)
    win = window(kp1, kp2, radius)
    g = np.zeros(len(kp2), bool)
    g[group] = True
    assert win[g].all()
    lo, hi = b[g].min(), b[g].max()
    other = win & ~g
    assert not (other & (b >= lo - 8) & (b <= hi + 8)).any(), "the gap is many bucket widths"
    first = int((other & (b < lo)).sum())
    last = int(win.sum()) - 1 - int((other & (b > hi)).sum())
    assert last - first + 1 == int(g.sum())
    return first, last


def union8_overflow(nu, c, K, family):
    """Queries match_union8_kernel hands to match_overflow_kernel, from the claims alone (the families' derivations above):
    every live query of a round whose list is longer than UCAP; otherwise the queries with more than K in radius and, in the
    flat family, those that need the rescue (three or more members) in a round whose list is longer than the SAD8 store."""
    n = 0
    for nu_r, c_r in zip(nu, c):
        if nu_r > UCAP:
            n += len(c_r)
        else:
            n += sum(1 for x in c_r if x > K or (family == "flat" and x >= 3 and nu_r > S8ROWS))
    return n


# ---------------------------------------------------------------- geometry
@functools.lru_cache(None)
def _diamond(rmax=40, xmin=-40, xmax=40):
    pts = [(dx, dy) for dx in range(xmin, xmax + 1) for dy in range(-rmax, rmax + 1) if abs(dx) + abs(dy) <= rmax]
    pts.sort(key=lambda p: (abs(p[0]) + abs(p[1]), p))
    return np.array(pts, int)


def _disjoint(sizes):
    """len(sizes) queries 400 apart in y, query k with its own cluster of sizes[k] targets within L1 40."""
    q = np.array([(QX, QY + 400 * k) for k in range(len(sizes))], int)
    clusters = [q[k] + _diamond()[:m] for k, m in enumerate(sizes)]
    far = np.array([(QX, QY - 1000)], int)
    return q, clusters, far


_A = np.array([(QX + 15, QY - 40)], int)   # within the radius of the first three of eight shared queries only


def _shared(nq, nu, fillers=0, tail=False):
    """nq = 1: one query and nu targets around it.  nq = 8: queries 10 apart in y around one cluster; from nu = 2 on one
    target (_A) is in radius of the first three queries only, so c = nu for those and nu - 1 for the others.  tail: the
    members' x is larger than every filler's.  Fillers (target 0 among them) are far below, at smaller x."""
    lo = 10 if tail else -20
    if nq == 1:
        q = np.array([(QX, QY)], int)
        mem = q[0] + _diamond(40, lo if tail else -40, 20 if tail else 40)[:nu]
        c = [nu]
    else:
        q = np.array([(QX, QY + 10 * k) for k in range(G)], int)
        main = np.array([(QX + dx, QY + 35 + dy) for dy in range(-8, 9) for dx in range(lo, 21)], int)
        na = 1 if nu >= 2 else 0
        mem = np.concatenate([_A[:na], main[:nu - na]])
        c = [nu] * 3 + [nu - na] * 5
    assert len(mem) == nu
    fil = np.array([(QX - 70 + i % 21, QY + 300 + 3 * i) for i in range(max(fillers, 1))], int)
    return q, mem, fil, c


# ---------------------------------------------------------------- descriptors
def _sads(d1, d2, i, members):
    return np.abs(d2[members].astype(np.int64) - d1[i].astype(np.int64)).sum(1)


def _clear(rng, M, need_planted, pick_ok=None, D=None, K=None):
    """A query with more than K in radius keeps its K nearest by (distance, index) (the reference's radius search): its best
    is planted on the LAST of those, the candidate the K-cap selection must not lose."""
    n1, n2 = M.shape
    d1 = rng.integers(-1000, 1001, (n1, DLEN))
    d2 = rng.integers(-1000, 1001, (n2, DLEN))
    planted = -np.ones(n1, int)
    used = set()
    for i in range(n1):
        mem = [t for t in np.flatnonzero(M[i]) if t not in used and (pick_ok is None or pick_ok[i, t])]
        if not mem:
            continue
        t = mem[(-1, 0, len(mem) // 2)[i % 3]]
        if K is not None and M[i].sum() > K:
            kept = sorted(np.flatnonzero(M[i]), key=lambda u: (D[i, u], u))[:K]
            t = [u for u in kept if u in mem][-1]
        v = d1[i].copy()
        pos = rng.permutation(DLEN)[:10 + i]
        v[pos] += np.where(v[pos] >= 1000, -1, 1)
        d2[t] = v
        planted[i] = t
        used.add(t)
    for i in range(n1):
        mem = np.flatnonzero(M[i])
        s = _sads(d1, d2, i, mem)
        if planted[i] >= 0:
            assert s[mem == planted[i]][0] == 10 + i and (s[mem != planted[i]] >= CLEAR_GAP).all(), "the 20000 gap"
        else:
            # a query without a best of its own (fewer shared members than queries): short lists only, no two SADs equal, so
            # whatever the rescue scores there is no tie to hand over
            assert not need_planted[i] and len(mem) <= S8ROWS and len(set(s.tolist())) == len(s) and (s >= CLEAR_GAP).all()
    return d1.astype(np.float32), d2.astype(np.float32), planted


def _flat_row(total, roll):
    assert 0 <= total <= 7 * DLEN
    v = np.zeros(DLEN, int)
    v[:total // 7] = 7
    if total % 7:
        v[total // 7] = total % 7
    return np.roll(v, roll)


def _flat(M, sums):
    n1, n2 = M.shape
    d1 = np.zeros((n1, DLEN), np.float32)
    d2 = np.stack([_flat_row(int(s), 5 * t) for t, s in enumerate(sums)]).astype(np.float32)
    assert d2.min() >= 0 and d2.max() <= 7
    for i in range(n1):
        mem = np.flatnonzero(M[i])
        s = _sads(d1, d2, i, mem)
        assert np.array_equal(s, np.asarray(sums)[mem]) and len(set(s.tolist())) == len(s), "distinct SADs: no tie"
    return d1, d2


def _params(K=250, second=1, radius=RADIUS):
    mp = MatchParams.temporal()
    mp.max_neighbors, mp.enforce_2nd_best, mp.radius = int(K), int(second), float(radius)
    return mp


def _assemble(name, seed, q, groups, sums, far, family, mp, claims, stereo=False, pick_ok_row=False):
    """Targets = far[0] (target 0), then the groups' and the other far keypoints in a seeded shuffle.  sums: the flat family's
    SAD per keypoint of every group (far keypoints get 5).  Returns the Case; claims gain family / K / ovf / groups."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate(list(groups) + [far[1:]])
    sm = np.concatenate([np.asarray(s, int) for s in sums] + [np.full(len(far) - 1, 5, int)])
    perm = rng.permutation(len(pts))
    kp2 = np.concatenate([far[:1], pts[perm]]).astype(np.float32)
    sm = np.concatenate([[5], sm[perm]])
    inv = np.empty(len(pts), int)
    inv[perm] = np.arange(len(pts)) + 1
    gidx, o = [], 0
    for g_ in groups:
        gidx.append(inv[o:o + len(g_)])
        o += len(g_)
    kp1 = np.asarray(q, np.float32)
    M = l1(kp1, kp2) <= np.float32(mp.radius)
    claims = dict(claims, family=family, K=int(mp.max_neighbors), groups=gidx)
    if family == "clear":
        need = np.zeros(len(kp1), bool)
        if not stereo:
            for r_, nu_r in zip(rounds_of(kp1), claims["nu"]):
                need[r_] = (M[r_].sum(1) >= 3) & (S8ROWS < nu_r <= UCAP)
        ok = (kp1[:, None, 1] == kp2[None, :, 1]) if pick_ok_row else None
        d1, d2, planted = _clear(rng, M, need, ok, l1(kp1, kp2), int(mp.max_neighbors))
        claims["planted"] = planted
    else:
        d1, d2 = _flat(M, sm)
    if not stereo and "ovf" not in claims:
        claims["ovf"] = union8_overflow(claims["nu"], claims["c"], claims["K"], family)
    return Case(name, kp1, kp2, d1, d2, mp, claims)


def _disjoint_sums(sizes):
    """Flat family: query 0's best stands clear (1 against 11: accepted at ratio 0.9), the others' two best are 10 and 11
    (rejected)."""
    return [[1 if (k == 0 and i == 0) else 10 + i for i in range(m)] for k, m in enumerate(sizes)]


def _shared_sums(nq, nu):
    return [[1] + [10 + i for i in range(nu - 1)]]


def _sizes(total, n=G):
    """n cluster sizes that sum to `total`, as equal as they get (the larger ones first)."""
    return [total // n + (1 if k < total % n else 0) for k in range(n)]


def disjoint_case(name, seed, sizes, family, K=250, second=1):
    q, clusters, far = _disjoint(sizes)
    rounds = [list(sizes[i:i + G]) for i in range(0, len(sizes), G)]
    claims = dict(W=sum(sizes) + 1, nu=[sum(r) for r in rounds], c=rounds)
    return _assemble(name, seed, q, clusters, _disjoint_sums(sizes), far, family, _params(K, second), claims)


def shared_case(name, seed, nq, nu, family, K=250, second=1, fillers=0, tail=False):
    q, mem, fil, c = _shared(nq, nu, fillers, tail)
    claims = dict(W=nu + len(fil), nu=[nu], c=[c])
    if tail:
        claims["member_pos"] = (len(fil), len(fil) + nu - 1)
    return _assemble(name, seed, q, [mem], _shared_sums(nq, nu), fil, family, _params(K, second), claims)


# ---------------------------------------------------------------- the cases, by capacity
def _seed(*k):
    """A seed from a case's name parts (not hash(): that one changes from run to run)."""
    return 4100 + sum((i + 1) * (j + 7) * ord(ch) for i, v in enumerate(k) for j, ch in enumerate(str(v)))


@functools.lru_cache(None)
def union_list_cases():
    out = []
    for fam in FAMILIES:
        for nu in (UCAP - 8, UCAP - 7, UCAP - 1, UCAP, UCAP + 1):
            out.append(disjoint_case(f"list-{nu}-{fam}", _seed("list", nu, fam), _sizes(nu), fam))
        out.append(disjoint_case(f"list-{UCAP}+{UCAP + 1}-{fam}", _seed("list2", fam), _sizes(UCAP) + _sizes(UCAP + 1), fam))
    return out


@functools.lru_cache(None)
def store_cases():
    out = [disjoint_case(f"store-{nu}-flat", _seed("store", nu), _sizes(nu), "flat") for nu in (S8ROWS - 1, S8ROWS, S8ROWS + 1, S8ROWS + 8)]
    out += [disjoint_case(f"store-{nu}-clear", _seed("store", nu, "c"), _sizes(nu), "clear") for nu in (S8ROWS + 1, 300, UCAP)]
    return out


PIPELINE_NU = (1, 2, 3, 8 * NP // 2 - 1, 8 * NP // 2, 8 * NP // 2 + 1, 8 * NP - 1, 8 * NP, 8 * NP + 1)


@functools.lru_cache(None)
def pipeline_cases():
    return [shared_case(f"pipe-q{nq}-nu{nu}-2nd{second}-{fam}", _seed("pipe", nq, nu, second, fam), nq, nu, fam, second=second)
            for fam in FAMILIES for second in (0, 1) for nq in (1, G) for nu in PIPELINE_NU]


WINDOW_MEMBERS = 20
WINDOW_W = (KPCAP - 1, KPCAP, KPCAP + 1, KPCAP + 8, KPCAP + 19, KPCAP + 20, KPCAP + 21, KPCAP + 31, KPCAP + 32, KPCAP + 33, KPCAP + 129,
            256, 257)


def one_row_case(fam):
    """Every keypoint of both images on one row: the target image's y range is empty (yscale = 0) and every window keypoint is
    a member of some query (nu == W).  Target 0 cannot be both on the row and out of every radius inside the window, so it is far
    away in x: the one case whose window is not the whole image (W == n2 - 1)."""
    n = 200
    q = np.array([(QX + 10 * k, QY) for k in range(G)], int)
    xs = np.array([x for x in range(QX - 50, QX + 121) if all(abs(abs(x - qx) - RADIUS) > 4 for qx in q[:, 0])])   # nobody on a radius
    tx = xs[(np.arange(n) * 37) % len(xs)]
    mem = np.stack([tx, np.full(n, QY)], 1)
    far = np.array([(QX + 4000, QY)], int)
    c = [int((np.abs(tx - x) <= RADIUS).sum()) for x in q[:, 0]]
    claims = dict(W=n, nu=[n], c=[c])
    return _assemble(f"window-one-row-{fam}", _seed("row", fam), q, [mem], [[1] + [10 + i for i in range(n - 1)]], far, fam, _params(), claims)


@functools.lru_cache(None)
def window_cases():
    out = []
    for fam in FAMILIES:
        for W in WINDOW_W:
            out.append(shared_case(f"window-{W}-{fam}", _seed("win", W, fam), G, WINDOW_MEMBERS, fam, fillers=W - WINDOW_MEMBERS, tail=True))
        out.append(one_row_case(fam))
    return out


@functools.lru_cache(None)
def kcap_cases():
    out = []
    for fam in FAMILIES:
        for K in (5, 250):
            for c in (K - 1, K, K + 1):
                out.append(shared_case(f"kcap-K{K}-c{c}-{fam}", _seed("k1", K, c, fam), 1, c, fam, K=K))
            for c in (K, K + 1):
                out.append(disjoint_case(f"kcap-K{K}-c{c}+1-{fam}", _seed("k2", K, c, fam), [c, 1], fam, K=K))
    return out


@functools.lru_cache(None)
def staging_cases():
    """One query with more in radius than a union list holds: match_overflow_kernel takes it whichever tile kernel ran."""
    out = []
    for K in (250, 5000):
        for c in (OVF_STAGE - 1, OVF_STAGE, OVF_STAGE + 1, 2 * OVF_STAGE + 1):
            out.append(shared_case(f"stage-K{K}-c{c}-clear", _seed("st", K, c), 1, c, "clear", K=K))
            if c <= 7 * DLEN - 10:
                out.append(shared_case(f"stage-K{K}-c{c}-flat", _seed("st", K, c, "f"), 1, c, "flat", K=K))
    return out


@functools.lru_cache(None)
def batch_cases():
    """match_batch_kernel's pair-list segment (matcher variant 2 where the build has it; valid inputs for every variant)."""
    return [disjoint_case(f"seg-{c}-{fam}", _seed("seg", c, fam), [c, 5, 1, 2], fam) for fam in FAMILIES for c in (MB_SEG - 1, MB_SEG, MB_SEG + 1)]


def rectified_F():
    from libviso_amd import hostmath, synth
    return hostmath.F_from_P(synth.KITTI_P1, synth.KITTI_P2)


def _stereo_params(K=200, second=0):
    mp = MatchParams.stereo(rectified_F())
    mp.max_neighbors, mp.enforce_2nd_best = int(K), int(second)
    return mp


def stereo_window_case(W, n_low=6, n_high=10, second=0):
    """One query; gate-passing targets on its row at the window's start (low x) and end (high x), off-row in-radius targets beside
    the low ones, far fillers between: with W > ST_WCAP the two groups sit in different chunks."""
    q = np.array([(QX, QY)], int)
    low = np.array([(QX - 70 + i, QY) for i in range(n_low)] + [(QX - 60 + i, QY + 12) for i in range(3)], int)
    high = np.array([(QX + 60 + i, QY) for i in range(n_high)], int)
    fil = np.array([(QX - 40 + i % 81, QY + 500 + i) for i in range(W - len(low) - len(high))], int)
    claims = dict(W=W, c=[len(low) + len(high)], row=[n_low + n_high], low_pos=(0, len(low) - 1), high_pos=(W - n_high, W - 1))
    return _assemble(f"stereo-window-{W}", _seed("sw", W), q, [low, high], [[0] * len(low), [0] * len(high)], fil, "clear",
                     _stereo_params(second=second), claims, stereo=True, pick_ok_row=True)


def stereo_slots_case(n_row):
    q = np.array([(QX, QY)], int)
    row = np.array([(QX - 30 + 5 * i, QY) for i in range(n_row)], int)
    off = np.array([(QX - 20 + 4 * i, QY + 12 + i) for i in range(10)], int)
    fil = np.array([(QX - 40 + i % 81, QY + 500 + i) for i in range(30)], int)
    claims = dict(W=n_row + 10 + 30, c=[n_row + 10], row=[n_row])
    return _assemble(f"stereo-slots-{n_row}", _seed("ss", n_row), q, [row, off], [[0] * n_row, [0] * 10], fil, "clear",
                     _stereo_params(second=1), claims, stereo=True, pick_ok_row=True)


def stereo_kcap_case(c, K=200):
    """A dense cluster: c in radius, those on the query's row (dy = 0 inside the diamond) pass the gate."""
    q = np.array([(QX, QY)], int)
    mem = q[0] + _diamond()[:c]
    fil = np.array([(QX - 40 + i % 81, QY + 500 + i) for i in range(20)], int)
    claims = dict(W=c + 20, c=[c], row=[int((mem[:, 1] == QY).sum())])
    return _assemble(f"stereo-kcap-K{K}-c{c}", _seed("sk", c), q, [mem], [[0] * c], fil, "clear", _stereo_params(K=K), claims,
                     stereo=True, pick_ok_row=True)


@functools.lru_cache(None)
def stereo_cases():
    out = [stereo_window_case(W) for W in (ST_WCAP - 1, ST_WCAP, ST_WCAP + 1, 2 * ST_WCAP + 1)]
    out += [stereo_slots_case(n) for n in (ST_SLOTS - 1, ST_SLOTS, ST_SLOTS + 1)]
    out += [stereo_kcap_case(c) for c in (199, 200, 201)]
    return out


TEMPORAL_GROUPS = {"union_list": union_list_cases, "store": store_cases, "pipeline": pipeline_cases, "window": window_cases,
                   "kcap": kcap_cases, "staging": staging_cases, "batch": batch_cases}
# groups whose overflow count is derived (match_union8_kernel only); staging and batch are results and counters only
OVF_DERIVED = ("union_list", "store", "pipeline", "window", "kcap")


def all_temporal():
    return [(g, c) for g, f in TEMPORAL_GROUPS.items() for c in f()]
