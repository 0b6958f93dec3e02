"""The loop-detection restatement (tests/loop_detect_ref_py.py) on its own, no GPU: the hand cases
in both of its forms, the literal form against the flat form on every query of the revisit
scenario, the conditions that scenario must meet for the GPU comparison to mean something, and the
summation-order case."""
import struct

import numpy as np
import pytest

import loop_detect_cases as C
import loop_detect_ref_py as R


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


@pytest.mark.parametrize("literal", [True, False], ids=["literal", "flat"])
@pytest.mark.parametrize("case", C.HAND_CASES, ids=lambda f: f.__name__)
def test_hand_case(case, literal):
    case(lambda scoring: R.RefLoop(scoring, literal))


@pytest.fixture(scope="module")
def scenario_runs():
    vectors, steps = C.scenario()
    seen = dict(words=0, score=0, cut=0, dup=0, equal_first=0)

    def tally(d):
        def on_step(k, r):
            t = d.trace if r["ran"] else {}
            seen["words"] += len(t.get("words_dropped", []))
            seen["score"] += len(t.get("score_dropped", []))
            seen["cut"] += len(t.get("cut_dropped", []))
            seen["dup"] += len(t.get("duplicates", []))
            f = list(t.get("first", {}).values())
            seen["equal_first"] += len(f) - len(set(f))
        return on_step

    flat = R.RefLoop(0, False)
    lit = R.RefLoop(0, True)
    rf = C.run_scenario(flat, vectors, steps, tally(flat))
    rl = C.run_scenario(lit, vectors, steps)
    return vectors, steps, rf, rl, seen


def test_literal_equals_flat(scenario_runs):
    _, _, rf, rl, _ = scenario_runs
    assert len(rf) == len(rl) == 120
    for k, (a, b) in enumerate(zip(rf, rl)):
        assert a["ran"] == b["ran"], k
        assert a["min_score"].tobytes() == b["min_score"].tobytes(), k
        assert a["candidates"] == b["candidates"], k
        assert a["enough"] == b["enough"], k
        assert a["groups"] == b["groups"], k


def test_scenario_is_not_vacuous(scenario_runs):
    _, steps, rf, _, seen = scenario_runs
    assert any(not r["ran"] for r in rf)                      # the early exit
    assert any(r["cleared"] for r in rf)                      # empty candidates clear groups
    assert seen["words"] > 0                                  # the common-word filter
    assert seen["score"] > 0                                  # minScore
    assert seen["cut"] > 0                                    # the 0.75 cut
    assert seen["dup"] > 0                                    # a duplicate pBestKF
    assert seen["equal_first"] > 0                            # two sharing keyframes, equal first
    assert any(c >= 3 for r in rf for _, c in r["groups"])    # a group counter of 3 or more
    assert sum(1 for r in rf if r["enough"]) >= 5
    assert any(r["double_match"] for r in rf)                 # one group, two previous groups
    assert any(st["erase"] for st in steps)
    assert any(len(c) > len(o) for st in steps[-1:]
               for c, o in zip(st["graph"]["conn"], st["graph"]["ordered"]))


@pytest.mark.parametrize("scoring", [0, 1], ids=["L1", "L2"])
def test_order_case_sums_differ(scoring):
    w, a, b = C.order_case()
    t = R.common_terms(w, a, w, b, scoring)
    terms = [x for _, _, x in t]
    seq = R.sum_sequential(terms)
    assert R.triple(w, a, w, b, scoring) == (len(w), 0, seq)
    assert bits(R.sum_reversed(terms)) != bits(seq)
    assert bits(R.sum_pairwise(terms)) != bits(seq)
    assert bits(R.sum_lane_strided([(j, x) for j, _, x in t])) != bits(seq)
