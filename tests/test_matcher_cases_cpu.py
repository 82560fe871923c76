"""The inputs of tests/test_gpu_matcher_capacity.py, proven on the plain model alone (tests/matcher_cases.py): every case
sits on the capacity it claims to sit on, the capacities are the ones the kernels are compiled with, and no case is vacuous
for the oracle.  Runs without a device."""
import os
import re

import numpy as np
import pytest

import matcher_cases as MC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libviso_amd", "csrc")


def _define(name, fname):
    with open(os.path.join(CSRC, fname)) as f:
        m = re.findall(r"^\s*#\s*define\s+%s\s+(\d+)\b" % re.escape(name), f.read(), re.M)
    assert m, f"{fname} no longer defines {name}"
    return {int(v) for v in m}


@pytest.mark.parametrize("cap", sorted(MC.CAPACITIES))
def test_capacities_are_the_kernels(cap):
    value, where, group = MC.CAPACITIES[cap]
    for name, fname in where:
        got = _define(name, fname)
        assert got == {value}, (f"{fname}: {name} = {sorted(got)}, tests/matcher_cases.py pins {cap} = {value}: "
                                f"edit {cap} there and move the '{group}' cases of tests/matcher_cases.py with it")
    # a list position must fit the 9 low bits of a tracker key, and the SAD8 store must hold whole pipeline iterations
    assert MC.UCAP + MC.PAD <= 512 and MC.S8ROWS % (8 * MC.NP) == 0 and MC.KPCAP % 128 == 0


def _ids(cases):
    return [c.name for c in cases]


TEMPORAL = [c for _, c in MC.all_temporal()]


@pytest.mark.parametrize("case", TEMPORAL, ids=_ids(TEMPORAL))
def test_temporal_claims(case):
    kp1, kp2, d1, d2, mp, claims = case
    got = MC.model(kp1, kp2, mp)
    assert got["W"] == claims["W"] and got["nu"] == claims["nu"] and got["c"] == claims["c"], (got, claims)
    assert len(kp1) <= MC.QPB and len(kp2) <= 1650
    assert np.array_equal(kp1, np.rint(kp1)) and np.array_equal(kp2, np.rint(kp2))            # integer coordinates
    if "one-row" in case.name:
        assert len(set(kp1[:, 1].tolist()) | set(kp2[:, 1].tolist())) == 1 and got["nu"] == [got["W"]] and got["W"] == len(kp2) - 1
    else:
        assert got["W"] == len(kp2) and len(set(kp1[:, 1].tolist())) == len(kp1)
    D = MC.l1(kp1, kp2)
    r = np.float32(mp.radius)
    assert not ((D > r - 4) & (D < r + 4)).any()                                               # nobody on the radius
    if "member_pos" in claims:
        assert MC.pos_bounds(kp1, kp2, mp.radius, claims["groups"][0]) == claims["member_pos"]
    assert claims["ovf"] == MC.union8_overflow(got["nu"], got["c"], mp.max_neighbors, claims["family"])
    # the descriptors fit the planes of shift 3 without clamping
    assert np.abs(np.concatenate([d1, d2])).max() <= (1000 if claims["family"] == "clear" else 7)
    assert mp.ratio_2nd_best == 0.9


def test_the_cases_reach_every_fork():
    nus = lambda f: [c.claims["nu"] for c in f()]                                           # noqa: E731
    U, S, P = MC.UCAP, MC.S8ROWS, 8 * MC.NP
    assert {(U - 8,), (U - 7,), (U - 1,), (U,), (U + 1,), (U, U + 1)} == {tuple(n) for n in nus(MC.union_list_cases)}
    for fam in MC.FAMILIES:
        assert {c.claims["ovf"] for c in MC.union_list_cases() if c.claims["family"] == fam} == ({0, 8} if fam == "clear" else {8, 16})
    flat = {c.claims["nu"][0]: c for c in MC.store_cases() if c.claims["family"] == "flat"}
    assert sorted(flat) == [S - 1, S, S + 1, S + 8] and all(min(c.claims["c"][0]) >= 3 for c in flat.values())
    assert [flat[n].claims["ovf"] for n in sorted(flat)] == [0, 0, 8, 8]
    clear = {c.claims["nu"][0]: c.claims["ovf"] for c in MC.store_cases() if c.claims["family"] == "clear"}
    assert clear == {S + 1: 0, 300: 0, U: 0}
    assert set(MC.PIPELINE_NU) == {1, 2, 3, P // 2 - 1, P // 2, P // 2 + 1, P - 1, P, P + 1} == {1, 2, 3, 7, 8, 9, 15, 16, 17}
    assert len(MC.pipeline_cases()) == 9 * 2 * 2 * 2 and all(c.claims["ovf"] == 0 for c in MC.pipeline_cases())
    tails = {(c.claims["W"] - MC.KPCAP) % 32 for c in MC.window_cases() if c.claims["W"] > MC.KPCAP}
    assert {0, 1, 31} <= tails
    ws = {c.claims["W"] for c in MC.window_cases()}
    assert {511, 512, 513, 543, 544, 545, 641, 256, 257} <= ws and {500, 511, 512, 513} <= {w - MC.WINDOW_MEMBERS for w in ws}
    for c in MC.window_cases():
        if "member_pos" in c.claims and c.claims["W"] in (520, 531):                          # members on both sides of position 512
            assert c.claims["member_pos"][0] < MC.KPCAP <= c.claims["member_pos"][1]
    assert all(c.claims["ovf"] == 0 for c in MC.window_cases() if c.claims["family"] == "clear")
    for K in (5, 250):
        k = {c.name: c.claims for c in MC.kcap_cases() if c.claims["K"] == K and c.claims["family"] == "clear"}
        assert [k[f"kcap-K{K}-c{c}-clear"]["ovf"] for c in (K - 1, K, K + 1)] == [0, 0, 1]
        assert k[f"kcap-K{K}-c{K}+1-clear"]["nu"] == [K + 1] and k[f"kcap-K{K}-c{K}+1-clear"]["ovf"] == 0
        assert k[f"kcap-K{K}-c{K + 1}+1-clear"]["ovf"] == 1
    assert {c.claims["c"][0][0] for c in MC.staging_cases()} == {MC.OVF_STAGE - 1, MC.OVF_STAGE, MC.OVF_STAGE + 1, 2 * MC.OVF_STAGE + 1}
    assert {c.claims["K"] for c in MC.staging_cases()} == {250, 5000}
    assert {c.claims["c"][0][0] for c in MC.batch_cases()} == {MC.MB_SEG - 1, MC.MB_SEG, MC.MB_SEG + 1}


STEREO = MC.stereo_cases()


@pytest.mark.parametrize("case", STEREO, ids=_ids(STEREO))
def test_stereo_claims(case):
    kp1, kp2, d1, d2, mp, claims = case
    got = MC.model_stereo(kp1, kp2, mp)
    assert got == {k: claims[k] for k in ("W", "c", "row")}, (got, claims)
    assert got["W"] == len(kp2) and mp.enforce_epipolar == 1
    if "low_pos" in claims:
        assert MC.pos_bounds(kp1, kp2, mp.radius, claims["groups"][0]) == claims["low_pos"]
        assert MC.pos_bounds(kp1, kp2, mp.radius, claims["groups"][1]) == claims["high_pos"]
    # a planted best on the query's own row: the gate lets it through
    t = claims["planted"][0]
    assert t > 0 and kp2[t, 1] == kp1[0, 1]


def test_the_stereo_cases_reach_every_fork():
    C, S = MC.ST_WCAP, MC.ST_SLOTS
    w = {c.claims["W"]: c.claims for c in MC.stereo_cases() if "low_pos" in c.claims}
    assert sorted(w) == [C - 1, C, C + 1, 2 * C + 1]
    chunks = lambda cl: {cl["low_pos"][0] // C, cl["low_pos"][1] // C, cl["high_pos"][0] // C, cl["high_pos"][1] // C}   # noqa: E731
    assert chunks(w[C - 1]) == chunks(w[C]) == {0} and chunks(w[C + 1]) == {0, 1} and chunks(w[2 * C + 1]) == {0, 1, 2}
    assert [c.claims["row"][0] for c in MC.stereo_cases() if "slots" in c.name] == [S - 1, S, S + 1]
    assert [(c.claims["c"][0], c.claims["K"]) for c in MC.stereo_cases() if "kcap" in c.name] == [(199, 200), (200, 200), (201, 200)]


def test_model_against_a_literal_loop():
    case = next(c for c in MC.union_list_cases() if len(c.kp1) == 16 and c.claims["family"] == "clear")
    kp1, kp2, _, _, mp, claims = case
    order = sorted(range(len(kp1)), key=lambda i: float(kp1[i, 1]))
    nu, cs = [], []
    for r0 in range(0, len(order), 8):
        seen, row = set(), []
        for i in order[r0:r0 + 8]:
            n = 0
            for t in range(len(kp2)):
                if abs(float(kp1[i, 0]) - float(kp2[t, 0])) + abs(float(kp1[i, 1]) - float(kp2[t, 1])) <= mp.radius:
                    n += 1
                    seen.add(t)
            row.append(n)
        nu.append(len(seen))
        cs.append(row)
    got = MC.model(kp1, kp2, mp)
    assert got["nu"] == nu == claims["nu"] and got["c"] == cs == claims["c"]


ALL = TEMPORAL + STEREO


@pytest.mark.parametrize("case", ALL, ids=_ids(ALL))
def test_no_case_is_vacuous_for_the_oracle(oracle, case):
    """At least one match everywhere; a rejected query wherever the flat family makes the ratio test decide between members
    the rescue has to score (queries that do not see the cluster's one clear best: every flat case of two or more queries
    with three or more members each).  A flat case of ONE query cannot have both a match and a reject: it has the match."""
    kp1, kp2, d1, d2, mp, claims = case
    m, scored = oracle.match_desc(kp1, kp2, d1, d2, mp, return_scored=True)
    assert len(m) >= 1 and scored >= len(m)
    if claims["family"] == "flat" and mp.enforce_2nd_best:
        with_two = sum(1 for r in claims["c"] for c in r if c >= 2)
        if len(kp1) > 1 and with_two >= 4:
            assert len(m) < sum(1 for r in claims["c"] for c in r if c >= 1), "nobody is rejected"
    if claims["family"] == "clear":
        planted = claims["planted"]
        if all(c <= mp.max_neighbors for r in (claims["c"] if isinstance(claims["c"][0], list) else [claims["c"]]) for c in r):
            got = dict(zip(m[:, 0].tolist(), m[:, 1].tolist()))                                 # the planted best is the match
            assert all(got.get(i) == t for i, t in enumerate(planted) if t >= 0)
