"""circle_table_kernel<LDS> behind viso_match_circle (csrc/circle.hip), the join of the per-call drop-in loop, at the sizes
where it changes path: the LDS and the global-scratch tables (tabn <= / > 6144), the 40 KB dynamic-LDS attribute switch
(tabn 1706 / 1707), one to three passes of its 1024-thread loop with the running offset carried across them, truncation
by `cap`, keys at CIRC_TAB_MAX and negative ones (the literal loops), keys and values outside the tables, a duplicate key
that only the last row reveals, and empty lists.  The lists come from tests/edge_inputs.py; return code, n, circ and pcl
must equal the oracle's exactly.  Each case first asserts, on the oracle alone, that it joins what it is meant to join."""
import numpy as np
import pytest

import libviso_amd

import edge_inputs as E

pytestmark = pytest.mark.gpu

CASES = E.circle_cases()
_want = {}


def _oracle(oracle, name):
    """The oracle's full answer for a case, computed once and left unchanged."""
    if name not in _want:
        lists = CASES[name]["lists"]
        r, circ, pcl, n = oracle.match_circle(*lists, cap=max(1, 4 * len(lists[0])))
        assert r == 1 and n == len(circ)
        for a in (circ, pcl):
            a.setflags(write=False)
        _want[name] = (circ, pcl, n)
    return _want[name]


def _compare(oracle, lists, cap):
    r0, c0, p0, n0 = oracle.match_circle(*lists, cap=cap)
    r1, c1, p1, n1 = libviso_amd.match_circle(*lists, cap=cap)
    assert (r1, n1) == (r0, n0)
    assert np.array_equal(c1, c0) and np.array_equal(p1, p0)
    return r1, c1, p1, n1


@pytest.mark.parametrize("name", [k for k, c in CASES.items() if not c.get("truncate")])
def test_circle_equals_oracle(viso, oracle, name):
    case = CASES[name]
    circ, pcl, n = _oracle(oracle, name)
    E.check_circle_joins(name, case, n)                 # the condition, on the oracle alone, first
    before = [a.copy() for a in case["lists"]]
    r1, c1, p1, n1 = _compare(oracle, case["lists"], max(1, 4 * len(case["lists"][0])))
    assert r1 == 1 and n1 == n and np.array_equal(c1, circ) and np.array_equal(p1, pcl)
    assert all(np.array_equal(a, b) for a, b in zip(case["lists"], before))


@pytest.mark.parametrize("which", ["n_out", "n_out-1", "1"])
@pytest.mark.parametrize("name", [k for k, c in CASES.items() if c.get("truncate")])
def test_circle_truncated_by_cap(viso, oracle, name, which):
    case = CASES[name]
    circ, pcl, n = _oracle(oracle, name)
    E.check_circle_joins(name, case, n)
    assert n >= 3
    cap = {"n_out": n, "n_out-1": n - 1, "1": 1}[which]
    r1, c1, p1, n1 = _compare(oracle, case["lists"], cap)
    assert n1 == n                                       # the needed count, whatever the cap
    assert r1 == (1 if cap >= n else -1)
    assert len(c1) == cap and np.array_equal(c1, circ[:cap]) and np.array_equal(p1, pcl[:cap])
