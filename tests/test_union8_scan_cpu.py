"""match_union8_kernel's scan step (phase 1), as a lane-by-lane numpy model: the mask assembly that swaps the two 32-target
steps' nibble registers against each other gives, in lanes 0..31 and 32..63, the masks the earlier assembly (one swap of a
register with itself per step) gave for steps a and b; the 64-lane append keeps the union list's order; and the scored-pair
accounting (ntest - ncnt, summed over the lanes that take part) has the same total, the wide-window tail's nibble split
included.  No device and no library."""
import numpy as np
import pytest

LANES, HALF = 64, 32
UCAP = 448


def permlane32_swap(a, b):
    """v_permlane32_swap a, b: a's lanes 32..63 and b's lanes 0..31 change places -> (new a, new b)."""
    a, b = np.asarray(a), np.asarray(b)
    return np.concatenate([a[:HALF], b[:HALF]]), np.concatenate([a[HALF:], b[HALF:]])


def popc(x):
    return np.array([bin(int(v)).count("1") for v in np.asarray(x).ravel()]).reshape(np.shape(x))


def mbcnt(mask_bits):
    """per lane: set bits of the ballot below the lane"""
    return np.concatenate([[0], np.cumsum(mask_bits)[:-1]]).astype(int)


def old_m8(m):
    """one step: both halves' nibbles of the SAME 32 targets; swap(m, m) -> the joined mask in every lane"""
    r0, r1 = permlane32_swap(m, m)
    return (r0 << 4) | r1


def new_m8(ma, mb):
    r0, r1 = permlane32_swap(ma, mb)
    return (r0 << 4) | r1


def old_iteration(ul, ucnt, ma, mb, pos):
    """two steps: lanes 0..31 append a's entries, then b's; returns (ucnt, per-lane set bits counted by lanes 0..31)"""
    m8a, m8b = old_m8(ma), old_m8(mb)
    ua, ub = (m8a != 0xff)[:HALF], (m8b != 0xff)[:HALF]   # the 32-bit ballots (the halves agree)
    assert np.array_equal((m8a != 0xff)[HALF:], ua) and np.array_equal((m8b != 0xff)[HALF:], ub)
    ca = int(ua.sum())
    for l in range(HALF):
        if ua[l]:
            ul[min(ucnt + mbcnt(ua)[l], UCAP - 1)] = (int(m8a[l]) << 24) | (int(pos[l]) << 7)
    for l in range(HALF):
        if ub[l]:
            ul[min(ucnt + ca + mbcnt(ub)[l], UCAP - 1)] = (int(m8b[l]) << 24) | (int(pos[HALF + l]) << 7)
    return ucnt + ca + int(ub.sum()), (popc(m8a) + popc(m8b))[:HALF]


def new_iteration(ul, ucnt, ma, mb, pos):
    """one joined step: all 64 lanes append at ucnt + mbcnt(64-bit ballot)"""
    m8 = new_m8(ma, mb)
    u = m8 != 0xff
    at = mbcnt(u)
    for l in range(LANES):
        if u[l]:
            ul[min(ucnt + at[l], UCAP - 1)] = (int(m8[l]) << 24) | (int(pos[l]) << 7)
    return ucnt + int(u.sum()), popc(m8)


def _nibbles(rng, density):
    """a step's register: lanes 0..31 the low half's nibble (queries 0..3) of targets 0..31, lanes 32..63 the high half's
    (queries 4..7) of the same targets; a set bit = NOT a member"""
    return np.where(rng.random((LANES, 4)) < density, 0, 1).dot([8, 4, 2, 1]).astype(np.int64)


@pytest.mark.parametrize("density", [0.0, 0.02, 0.3, 1.0])
def test_joined_mask_is_step_a_below_and_step_b_above(density):
    rng = np.random.default_rng(int(density * 100) + 5)
    for _ in range(50):
        ma, mb = _nibbles(rng, density), _nibbles(rng, density)
        m8 = new_m8(ma, mb)
        assert np.array_equal(m8[:HALF], old_m8(ma)[:HALF])
        assert np.array_equal(m8[HALF:], old_m8(mb)[:HALF])
        # bit 7 - k = query k: the high nibble is the low half's (queries 0..3)
        assert np.array_equal(m8[:HALF] >> 4, ma[:HALF]) and np.array_equal(m8[:HALF] & 15, ma[HALF:])
        assert np.array_equal(m8[HALF:] >> 4, mb[:HALF]) and np.array_equal(m8[HALF:] & 15, mb[HALF:])


@pytest.mark.parametrize("density,iters", [(0.02, 6), (0.3, 4), (1.0, 9), (0.0, 3)])
def test_append_keeps_the_list_order_and_the_scored_total(density, iters):
    """several iterations in a row (density 1.0 over 9 iterations runs past UCAP: the clamp piles up in the last entry in
    both versions, and ucnt, the hand-over's input, is the same)"""
    rng = np.random.default_rng(iters * 10 + int(density * 7))
    ul_o, ul_n = np.zeros(UCAP, np.int64), np.zeros(UCAP, np.int64)
    uo = un = 0
    ntest_o = ntest_n = members = 0
    ncnt_o, ncnt_n = np.zeros(HALF, int), np.zeros(LANES, int)
    where = rng.permutation(LANES * iters)           # the staged window's positions, every one once
    for it in range(iters):
        ma, mb = _nibbles(rng, density), _nibbles(rng, density)
        members += int((4 - popc(ma)).sum() + (4 - popc(mb)).sum())   # (query, target) pairs in radius
        pos = where[it * LANES:(it + 1) * LANES]    # s_ypos[base + lane]: a's 32 positions, then b's
        uo, c_o = old_iteration(ul_o, uo, ma, mb, pos)
        un, c_n = new_iteration(ul_n, un, ma, mb, pos)
        ncnt_o += c_o
        ncnt_n += c_n
        ntest_o += 16                                  # lanes 0..31: two steps of eight tests
        ntest_n += 8                                   # every lane: eight tests of its own target
        assert uo == un
    keep = min(uo, UCAP)
    assert np.array_equal(ul_o[:keep], ul_n[:keep])
    if uo <= UCAP:
        assert len(set((ul_n[:keep] >> 7) & 0x1ffff)) == keep   # every member once
    scored_o = int((ntest_o - ncnt_o).sum())           # half == 0 adds ntest - ncnt
    scored_n = int((ntest_n - ncnt_n).sum())           # all 64 lanes add
    assert scored_o == scored_n == members


@pytest.mark.parametrize("density", [0.0, 0.1, 1.0])
def test_tail_step_of_32_with_each_half_counting_its_own_nibble(density):
    """the wide-window tail keeps its step of 32 targets with the joined mask in every lane: the earlier version let lanes
    0..31 count all eight bits (ntest += 8); now each half counts its own four queries' bits (ntest += 4) in all 64 lanes"""
    rng = np.random.default_rng(int(density * 10) + 77)
    for _ in range(30):
        m = _nibbles(rng, density)
        m8 = old_m8(m)                                  # swap(m, m): the same value in both halves
        assert np.array_equal(m8[:HALF], m8[HALF:])
        old = int((8 - popc(m8[:HALF])).sum())
        half = np.arange(LANES) >> 5
        own = popc(m8 & np.where(half == 1, 0x0f, 0xf0))
        assert np.array_equal(own[:HALF], popc(m[:HALF])) and np.array_equal(own[HALF:], popc(m[HALF:]))
        assert int((4 - own).sum()) == old


def test_tail_joined_to_64_targets_keeps_window_order():
    """a tail joined like the main loop (steps a and b = window positions base + 0..31 and base + 32..63): the same entries in
    the same order as two steps of 32"""
    rng = np.random.default_rng(3)
    for W in (513, 543, 544, 545, 575, 576, 577):
        ul_o, ul_n = np.zeros(UCAP, np.int64), np.zeros(UCAP, np.int64)
        uo = un = 0
        for base in range(512, W, 64):
            w = base + np.arange(LANES)
            ma, mb = _nibbles(rng, 0.2), _nibbles(rng, 0.2)
            ma[np.tile(w[:HALF] >= W, 2)] = 15          # past the window: NaN targets, nobody's member
            mb[np.tile(w[HALF:] >= W, 2)] = 15
            uo, _ = old_iteration(ul_o, uo, ma, mb, w)
            un, _ = new_iteration(ul_n, un, ma, mb, w)
        assert uo == un and np.array_equal(ul_o[:uo], ul_n[:un])
        assert (np.diff((ul_n[:un] >> 7) & 0x1ffff) > 0).all()
