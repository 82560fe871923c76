"""numpy restatement of include/viso_hip.h, "loop closure": place signatures, scores and candidates, the wide match.  Every function
exists twice: the form the tests compare the device with, and a slower one written another way (*_slow) that test_loops_cpu.py holds
it to."""
import numpy as np

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
SAD_MAX = (1 << 18) - 2     # every key sad << 14 | index stays below the all-ones "none"
DESC_LEN = 121


def splitmix64(state):
    """(draw, next state) of viso_splitmix64 (csrc/solver_dev.h)."""
    state = (state + GOLD) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31), state


def sign_draws(seed, bits):
    """[bits][2] Python ints: the two draws of every bit's stream."""
    out = []
    for b in range(bits):
        s = (seed * GOLD + b) & M64
        d0, s = splitmix64(s)
        d1, s = splitmix64(s)
        out.append((d0, d1))
    return out


def sign_table(seed, bits):
    """c [bits][121] of +-1."""
    c = np.empty((bits, DESC_LEN), np.int64)
    for b, draws in enumerate(sign_draws(seed, bits)):
        for k in range(DESC_LEN):
            c[b, k] = 1 if (draws[k // 64] >> (k % 64)) & 1 else -1
    return c


def words(rows, seed, bits):
    rows = np.asarray(rows, np.int64).reshape(-1, DESC_LEN)
    p = rows @ sign_table(seed, bits).T
    return ((p > 0).astype(np.int64) << np.arange(bits)).sum(1)


def words_slow(rows, seed, bits):
    draws = sign_draws(seed, bits)
    out = []
    for row in np.asarray(rows).reshape(-1, DESC_LEN):
        w = 0
        for b in range(bits):
            p = 0
            for k in range(DESC_LEN):
                p += int(row[k]) if (draws[b][k // 64] >> (k % 64)) & 1 else -int(row[k])
            w |= (1 if p > 0 else 0) << b
        out.append(w)
    return np.array(out, np.int64)


def signatures(desc, n, seed, bits):
    """uint8 [nf][2^bits] of desc [nf][cap][121] and counts n [nf]."""
    out = np.zeros((len(n), 1 << bits), np.uint8)
    for f in range(len(n)):
        out[f] = np.minimum(np.bincount(words(desc[f][:n[f]], seed, bits), minlength=1 << bits), 255)
    return out


def signatures_slow(desc, n, seed, bits):
    out = np.zeros((len(n), 1 << bits), np.uint8)
    for f in range(len(n)):
        for w in words_slow(desc[f][:n[f]], seed, bits):
            if out[f, w] < 255:
                out[f, w] += 1
    return out


def scores(sig, j0=0):
    """uint32 [n - j0][n]: s(j, i) for i <= j, 0 above the diagonal; by the SAD identity (sum + sum - SAD) / 2."""
    h = np.asarray(sig, np.int64)
    n = len(h)
    tot = h.sum(1)
    out = np.zeros((n - j0, n), np.uint32)
    for j in range(j0, n):
        sad = np.abs(h[:j + 1] - h[j]).sum(1)
        out[j - j0, :j + 1] = (tot[j] + tot[:j + 1] - sad) // 2
    return out


def scores_slow(sig, j0=0):
    h = np.asarray(sig, np.int64)
    n = len(h)
    out = np.zeros((n - j0, n), np.uint32)
    for j in range(j0, n):
        for i in range(j + 1):
            out[j - j0, i] = np.minimum(h[j], h[i]).sum()
    return out


def sequence_sums(sig, seq_len):
    """S [n][n] (int64; entries above the diagonal are not meaningful)."""
    s = scores(sig).astype(np.int64)
    n = len(s)
    S = np.zeros((n, n), np.int64)
    for k in range(seq_len):
        S[k:, k:] += s[:n - k, :n - k]
    return S


def candidates(sig, j0=0, min_gap=50, seq_len=1, nms=4, min_score=0, k=4):
    """(cand int32 [n - j0][k] filled with -1, score uint32 [n - j0][k])."""
    S = sequence_sums(sig, seq_len)
    n = len(S)
    cand, score = np.full((n - j0, k), -1, np.int32), np.zeros((n - j0, k), np.uint32)
    for j in range(j0, n):
        hi = j - min_gap
        if hi < 0:
            continue
        row = S[j, :hi + 1].copy()
        alive = row >= min_score
        for r in range(k):
            if not alive.any():
                break
            i = int(np.argmax(np.where(alive, row, -1)))    # the first of the largest: the lowest i
            cand[j - j0, r], score[j - j0, r] = i, row[i]
            alive[max(0, i - nms):i + nms + 1] = False
    return cand, score


def candidates_slow(sig, j0=0, min_gap=50, seq_len=1, nms=4, min_score=0, k=4):
    s = scores_slow(sig)
    n = len(s)
    cand, score = np.full((n - j0, k), -1, np.int32), np.zeros((n - j0, k), np.uint32)
    for j in range(j0, n):
        order = []
        for i in range(0, j - min_gap + 1):
            S = 0
            for q in range(seq_len):
                if i - q >= 0:
                    S += int(s[j - q, i - q])
            if S >= min_score:
                order.append((-S, i))
        order.sort()
        picked = []
        for negS, i in order:
            if len(picked) == k:
                break
            if all(abs(i - p) > nms for p in picked):
                cand[j - j0, len(picked)], score[j - j0, len(picked)] = i, -negS
                picked.append(i)
    return cand, score


def sad_matrix(Q, T):
    Q, T = np.asarray(Q, np.int64).reshape(-1, DESC_LEN), np.asarray(T, np.int64).reshape(-1, DESC_LEN)
    out = np.empty((len(Q), len(T)), np.int64)
    for q in range(len(Q)):
        out[q] = np.abs(T - Q[q]).sum(1)
    return np.minimum(out, SAD_MAX)


def wide_match_pair(Q, T, ratio):
    """int32 [m][3]: the accepted (q, t1, d1) in ascending q."""
    D = sad_matrix(Q, T)
    nq, nt = D.shape
    if nq == 0 or nt == 0:
        return np.zeros((0, 3), np.int32)
    t1 = D.argmin(1)                      # the first of the least: the lower index
    d1 = D[np.arange(nq), t1]
    if nt > 1:
        rest = D.copy()
        rest[np.arange(nq), t1] = np.iinfo(np.int64).max
        d2 = rest.min(1).astype(np.float64)
    else:
        d2 = np.full(nq, np.inf)
    qbest = D.argmin(0)
    keep = (d1.astype(np.float64) < d2 * np.float64(ratio)) & (qbest[t1] == np.arange(nq))
    return np.stack([np.arange(nq), t1, d1], 1)[keep].astype(np.int32)


def wide_match_pair_slow(Q, T, ratio):
    Q, T = np.asarray(Q).reshape(-1, DESC_LEN), np.asarray(T).reshape(-1, DESC_LEN)
    sad = [[min(sum(abs(int(a) - int(b)) for a, b in zip(Q[q], T[t])), SAD_MAX) for t in range(len(T))] for q in range(len(Q))]
    out = []
    for q in range(len(Q)):
        if not len(T):
            break
        t1 = min(range(len(T)), key=lambda t: (sad[q][t], t))
        d1 = sad[q][t1]
        d2 = min([sad[q][t] for t in range(len(T)) if t != t1], default=float("inf"))
        mutual = min(range(len(Q)), key=lambda p: (sad[p][t1], p)) == q
        if float(d1) < float(d2) * float(ratio) and mutual:
            out.append((q, t1, d1))
    return np.array(out, np.int32).reshape(-1, 3)


def wide_match(desc, n, pairs, ratio):
    return [wide_match_pair(desc[q][:n[q]], desc[t][:n[t]], ratio) for q, t in np.reshape(pairs, (-1, 2))]
