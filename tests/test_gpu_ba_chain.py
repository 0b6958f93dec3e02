"""The local BA's kernel chain keeps its bits: the heavy (wave per point) and light (thread per
point) points of k_ba2_lin and k_ba2_p4 run in one launch each, their workgroup partials rebuilt
from a per-point array by k_ba2_kfsum and by k_ba2_p4's last workgroup.  Every output of
ctx.local_bundle_adjustment must equal, bit for bit, what the commit before that change computed
(tests/golden/ba_chain_golden.npz, recorded by tools/make_golden_ba_chain.py on that commit), and
agree with the CPU oracle as in test_gpu_localmap.py (counts and erase flags exact, poses and
points within 1e-4), so a wrong golden cannot hide.

Graphs (tests/ba_chain_cases.py), each asserted to have the property it is there for:
  rejected_trial  889 edges, 178 heavy and 122 light points, a rejected trial (the iteration's next
                  trial runs on the kept linearisation)
  two_chunks      4,417 edges, six points with more than 64 edges (two 64-edge chunks per wave)
  three_chunks    6,649 edges, ten points with more than 128 edges
  wg_boundary     257 points: one full point workgroup and one point in the next; 128 light, 129
                  heavy (a misplaced partial-sum boundary shows here)
  no_heavy        95 edges, no heavy point (no heavy workgroup in the grids)
  no_light        no light point
and the 257-point graph solved again on the same context after the 140-keyframe one (the ticket
counter's reset, stale per-point entries of the reused workspace)."""
import os

import numpy as np
import pytest

import ba_chain_cases as C
from ba_problems import BF
from synth_problems import K_KITTI

pytestmark = pytest.mark.gpu
TOL = 1e-4  # test_gpu_localmap.py's
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_chain_golden.npz")


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(nfeatures=2000, max_batch=8))
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _check_golden(golden, name, P, got):
    assert str(golden[name + ".sha256"]) == C.input_digest(P), \
        "%s: the generated graph differs from the one the golden was recorded on (ba_problem or " \
        "its random generator changed); record again on the yardstick commit" % name
    T, X, er, st = got
    assert np.array_equal(C.stats_array(st), golden[name + ".stats"]), \
        (name, st, golden[name + ".stats"])
    assert np.array_equal(er, golden[name + ".erase"]), name
    assert np.array_equal(T, golden[name + ".T"]), (name, np.abs(T - golden[name + ".T"]).max())
    assert np.array_equal(X, golden[name + ".X"]), (name, np.abs(X - golden[name + ".X"]).max())


def _check_oracle(oracle_mod, P, got):
    T, X, er, st = got
    To, Xo, eo, so = oracle_mod.local_ba(P, K_KITTI, BF)
    assert st == so, (st, so)
    assert np.array_equal(er, eo), (np.nonzero(er != eo)[0][:10], er.sum(), eo.sum())
    assert np.abs(T - To).max() < TOL
    assert np.abs(X - Xo).max() < TOL
    return so


def _solve_and_check(ctx, oracle_mod, golden, name):
    P = C.problem(name)
    got = ctx.local_bundle_adjustment(P)
    _check_golden(golden, name, P, got)
    so = _check_oracle(oracle_mod, P, got)
    return P, C.edges_per_point(P), so


def test_rejected_trial(ctx, oracle_mod, golden):
    P, n, so = _solve_and_check(ctx, oracle_mod, golden, "rejected_trial")
    assert len(P["pt"]) == 889
    assert ((n > C.HEAVY).sum(), (n <= C.HEAVY).sum()) == (178, 122)
    assert so["iterations"] == (5, 10) and so["trials"] == (6, 10)
    assert sum(so["trials"]) > sum(so["iterations"])


def test_two_chunks(ctx, oracle_mod, golden):
    P, n, so = _solve_and_check(ctx, oracle_mod, golden, "two_chunks")
    assert len(P["pt"]) == 4417
    assert (n > 64).sum() == 6 and n.max() <= 128
    assert so["iterations"] == (5, 7)


def test_three_chunks(ctx, oracle_mod, golden):
    P, n, so = _solve_and_check(ctx, oracle_mod, golden, "three_chunks")
    assert len(P["pt"]) == 6649
    assert (n > 128).sum() == 10
    assert so["iterations"] == (5, 6)


def test_workgroup_boundary(ctx, oracle_mod, golden):
    P, n, so = _solve_and_check(ctx, oracle_mod, golden, "wg_boundary")
    assert len(P["X"]) == 257
    assert ((n <= C.HEAVY).sum(), (n > C.HEAVY).sum()) == (128, 129)
    assert so["iterations"] == (5, 10)


def test_no_heavy_point(ctx, oracle_mod, golden):
    P, n, _ = _solve_and_check(ctx, oracle_mod, golden, "no_heavy")
    assert len(P["pt"]) == 95
    assert n.max() <= C.HEAVY


def test_no_light_point(ctx, oracle_mod, golden):
    P, n, _ = _solve_and_check(ctx, oracle_mod, golden, "no_light")
    assert n.min() > C.HEAVY


def test_repeat_after_larger_graph(ctx, golden):
    """257 points, then 140 keyframes, then 257 points again on one context: the first and the
    third result bit-identical (and each the golden's)."""
    Pa, Pb = C.problem("wg_boundary"), C.problem("three_chunks")
    first = ctx.local_bundle_adjustment(Pa)
    mid = ctx.local_bundle_adjustment(Pb)
    third = ctx.local_bundle_adjustment(Pa)
    for a, b in zip(first[:3], third[:3]):
        assert np.array_equal(a, b)
    assert first[3] == third[3]
    _check_golden(golden, "wg_boundary", Pa, first)
    _check_golden(golden, "three_chunks", Pb, mid)
