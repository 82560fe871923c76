"""The travel field of include/viso_hip.h ("TSDF travel field") restated in numpy and heapq: the free cells from the distance field of
tests/field_ref.py, and the costs by Dijkstra's algorithm with a heap over the 26 moves, written literally.  No tiles, no sweeps and
no rounds: a mistake in the device's relaxation cannot be shared with this file.

  1. Box, states, sites and sq: field_ref.field with the same min_weight and flags.
  2. Free: (state & 3) != 2, not a site, sq >= clearance_sq (NONE is at least anything; clearance_sq < NONE).
  3. Goals: absolute voxel indices; one outside the box or in a cell that is not free is skipped; n_goals_used counts the entries
     of the list that were used.
  4. Moves: between free cells that are neighbours in the box, one of the 26; 3, 4 or 5 when 1, 2 or 3 indices change.
  5. cost[c]: the smallest sum over the sequences of moves from c to a used goal, NONE where c is not free or there is none.

path(cost, start): from a cell of finite cost to the first neighbour n with cost[n] + w == cost[c], in the order of
itertools.product((-1, 0, 1), repeat=3) without (0, 0, 0), until the cost is 0.

No device and no library at module level."""
import heapq
import itertools

import numpy as np

import field_ref as F

NONE = F.NONE
MAX_GOALS = 65536
MOVES = [e for e in itertools.product((-1, 0, 1), repeat=3) if e != (0, 0, 0)]


def move_cost(e):
    return 2 + sum(1 for v in e if v != 0)


def free_of(sq, state, flags, clearance_sq):
    """bool, the shape of sq: rule 2."""
    assert 0 <= clearance_sq < NONE
    return ((state & 3) != 2) & ~F.sites_of(state, flags) & (sq.astype(np.int64) >= clearance_sq)


def costs(free, goals_idx):
    """(cost uint32 of the shape of `free`, n_goals_used): rules 3 to 5 for goals given as cell indices of the box (any integers:
    one outside the box is skipped)."""
    n = free.shape
    assert 1 <= len(goals_idx) <= MAX_GOALS
    # the box with a rim of one cell that is not free around it, flat: a move is one addition, and the rim ends every move that
    # would leave the box
    p1, p2 = n[1] + 2, n[2] + 2
    rimmed = np.zeros((n[0] + 2, p1, p2), bool)
    rimmed[1:-1, 1:-1, 1:-1] = free
    is_free = rimmed.reshape(-1).tolist()
    steps = [((e[0] * p1 + e[1]) * p2 + e[2], move_cost(e)) for e in MOVES]
    best = {}
    heap = []
    used = 0
    for g in goals_idx:
        g = tuple(int(v) for v in g)
        if all(0 <= g[i] < n[i] for i in range(3)) and free[g]:
            used += 1
            c = ((g[0] + 1) * p1 + g[1] + 1) * p2 + g[2] + 1
            if c not in best:
                best[c] = 0
                heap.append((0, c))
    heapq.heapify(heap)
    while heap:
        d, c = heapq.heappop(heap)
        if d > best[c]:
            continue
        for step, w in steps:
            m = c + step
            if is_free[m] and d + w < best.get(m, NONE):
                best[m] = d + w
                heapq.heappush(heap, (d + w, m))
    out = np.full(rimmed.shape, NONE, np.uint32)
    if best:
        out.reshape(-1)[list(best)] = list(best.values())
    return np.ascontiguousarray(out[1:-1, 1:-1, 1:-1]), used


def travel(entries, min_weight, box, flags, clearance_sq, goals):
    """(cost, sq, state, n_goals_used, n_reached) of viso_tsdf_travel_field; goals: absolute voxel indices [n][3]."""
    sq, st, _ = F.field(entries, min_weight, box, flags)
    lo, _ = F.shape_of(box)
    cost, used = costs(free_of(sq, st, flags, clearance_sq), np.asarray(goals, np.int64).reshape(-1, 3) - lo)
    return cost, sq, st, used, int((cost != NONE).sum())


def path(cost, start):
    """The cells from `start` (a cell index of the box) to a goal as an int64 [m][3] array, or None when start is outside the box or
    its cost is NONE."""
    n = cost.shape
    c = tuple(int(v) for v in start)
    if not all(0 <= c[i] < n[i] for i in range(3)) or cost[c] == NONE:
        return None
    cells = [c]
    while cost[c] != 0:
        for e in MOVES:
            m = (c[0] + e[0], c[1] + e[1], c[2] + e[2])
            if all(0 <= m[i] < n[i] for i in range(3)) and cost[m] != NONE and int(cost[m]) + move_cost(e) == int(cost[c]):
                c = m
                break
        else:
            raise AssertionError(f"no neighbour of {c} leads on: not the costs of a travel field")
        cells.append(c)
    return np.array(cells, np.int64)
