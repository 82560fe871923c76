"""The inputs of tests/test_gpu_extract_rows.py and tests/test_gpu_circle_edges.py, checked on the oracle alone: the probe
of the packed rows lets no keypoint escape, and the circle cases join what they are meant to join.  The GPU tests assert
the same conditions before they compare; here they run without a device."""
import numpy as np
import pytest

import edge_inputs as E


def _extract_params():
    out = [(s, n) for s in E.SHAPES for n in E.COUNTS] + [(E.SHAPES[0], n) for n in E.EXTRA_COUNTS]
    return out


@pytest.mark.parametrize("shape,count", _extract_params(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_every_probe_keypoint_is_matched(oracle, shape, count):
    for pad in E.CAP_PADS:
        case = E.extract_case(shape, count, pad)
        assert case["cap"] == count + 1 + pad and (case["n"] == count + 1).all()
        assert (case["kp"][:, :, count + 1:] == E.FAR).all()
        _, lists = E.extract_expected(oracle, case)
        E.check_probe_is_full(case, lists)
        if pad:      # the cap changes nothing the oracle sees
            assert all(np.array_equal(lists[k][0], first[k][0]) and lists[k][1] == first[k][1] for k in lists)
        first = lists


def test_positions_cover_the_edges():
    """The position set holds what the kernel's conditions need, on the shape where nothing has to be dropped."""
    rows, cols = E.SHAPES[0]
    pts = set(E.position_set(rows, cols))
    for x in (0, cols - 1):
        for y in (0, rows - 1):
            assert (x, y) in pts
    xs, ys = {p[0] for p in pts}, {p[1] for p in pts}
    for d in range(8):
        assert {d, cols - 1 - d} <= xs and {d, rows - 1 - d} <= ys
    for d in range(1, 9):
        assert {-d, cols - 1 + d} <= xs and {-d, rows - 1 + d} <= ys
    assert {5.5, 6.5, cols - 6.5, cols - 5.5} <= xs and {5.5, 6.5, rows - 6.5, rows - 5.5} <= ys
    assert (E.FAR, E.FAR) in pts and (-E.FAR, -E.FAR) in pts
    assert max(abs(v) for p in pts for v in p) <= E.FAR
    # 257 keypoints hold the whole set of every shape; every tiny shape keeps its corners and the outside ring
    for rows, cols in E.SHAPES:
        base = E.position_set(rows, cols)
        have = {tuple(p) for p in E.positions(rows, cols, 257, 1).tolist()}
        assert set(base) <= have
        assert {(0, 0), (cols - 1, 0), (0, rows - 1), (cols - 1, rows - 1)} <= have
        assert all((-d, -d) in have and (cols - 1 + d, rows - 1 + d) in have for d in range(1, 9))


@pytest.mark.parametrize("shape", [E.SHAPES[0], E.SHAPES[1]], ids=str)
def test_ragged_probe(oracle, shape):
    for pad in E.CAP_PADS:
        case = E.extract_case(shape, E.RAGGED_COUNTS, pad)
        assert np.array_equal(case["n"], E.RAGGED_COUNTS + 1)
        _, lists = E.extract_expected(oracle, case)
        E.check_probe_is_full(case, lists)     # every index below the smaller n of a pair appears


def test_column_images_reach_the_full_range(oracle):
    case = E.extract_case(E.SHAPES[0], 65, 0, kind="columns")
    assert set(np.unique(case["images"]).tolist()) == {0, 255}
    desc, lists = E.extract_expected(oracle, case)
    E.check_probe_is_full(case, lists)
    assert desc.max() == 1020 and desc.min() == -1020


def test_circle_cases_join(oracle):
    cases = E.circle_cases()
    sizes = set()
    for name, case in cases.items():
        lists = case["lists"]
        r, circ, pcl, n = oracle.match_circle(*lists, cap=max(1, 4 * len(lists[0])))
        assert r == 1 and n == len(circ), name
        E.check_circle_joins(name, case, n)
        keys = np.concatenate([a[:, 0] for a in lists[1:]])
        if case["table"]:
            assert keys.min() >= 0 and keys.max() < E.CIRC_TAB_MAX
            sizes.add(int(keys.max()) + 1)
        if case["table"] is False:
            dup = any(len(np.unique(a[:, 0])) != len(a) for a in lists[1:])
            assert dup or keys.min() < 0 or keys.max() >= E.CIRC_TAB_MAX, name
        assert max(len(a) for a in lists) <= 3000
        if case["table"] is False:
            assert max(len(a) for a in lists[1:]) <= 300, name
    assert {1, 1706, 1707, 6143, 6144, 6145, 20000, E.CIRC_TAB_MAX} <= sizes
