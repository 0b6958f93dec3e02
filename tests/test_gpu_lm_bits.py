"""The D1 / D2 / D3 solves keep their bits through changes to csrc/mmt_lm.hip that are meant to
leave the arithmetic alone (first of them: g2o's LM step policy moved to csrc/mmt_lmstep.h, the
LDS-resident D1 fallback removed).  Every output of ctx.flow_solve and ctx.pose_optimization on
the cases of tests/lm_bits_cases.py must equal, bit for bit, what the commit before that change computed
(tests/golden/lm_solves_golden.npz, recorded by tools/make_golden_lm_solves.py on that commit), and
agree with the CPU oracle as in test_gpu_track.py (pose within 1e-4; inliers, iterations and
outlier flags exact), so a wrong golden cannot hide.

The cases are the smallest shapes at which each path can go wrong: the flow solve at 3 edges, one
wave with Huber-active edges (no closed-form Schur sums), the wave boundary (64 / 65), one item
per thread against two (256 / 257), the first item in the global item arrays (513), rejection
chains served from the candidate table (also with MMT_LM_MAX_CAND=1), the split solve with empty
slices, three groups, and a rejection chain across workgroups (slices of at most 256 edges), and
slices of two register items per thread on both sides of their run-time choice, each on a
Huber-active and on a clean system: 2 x 257 edges (the fused trial through the tile) and 2 x 513
(above 512 per slice: the two-pass trial with an exchange per pass, one item per slice in the
global item arrays); D1 at 3 and 8 edges (one round),
mixed and all-mono edges, and both sides of the 1024- and 2048-edge kernel thresholds (2049 is the
only way into the global-scratch kernel k_pose_opt)."""
import os

import numpy as np
import pytest

import lm_bits_cases as C
from synth_problems import K_KITTI

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-4  # test_gpu_track.py's
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_solves_golden.npz")


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


def _check_golden(golden, case, arrays, got):
    name = case["name"]
    assert str(golden[name + ".sha256"]) == C.input_digest(case, arrays), \
        "%s: the generated problem differs from the one the golden was recorded on " \
        "(synth_problems or its random generator changed); record again on the yardstick " \
        "commit" % name
    for k, v in got.items():
        g = golden["%s.%s" % (name, k)]
        assert v.dtype == g.dtype and np.array_equal(v, g), (name, k, v, g)


def _check_oracle(oracle_mod, case, arrays, got):
    if case["kind"] == "flow":
        rc, pose_o, st_o = oracle_mod.flow_solve(*arrays, *case["args"], K_KITTI)
        status, iterations, inliers = got["stats"].tolist()
        assert status == rc == 0
        assert np.abs(got["pose"] - pose_o).max() < POSE_TOL
        assert inliers == st_o["inliers"]
        if case["n"] >= 10:
            # as test_flow_solve_matches_oracle: a 3-edge problem is barely constrained and its
            # stop test flips on last-bit differences of the reduction order
            assert iterations == st_o["iterations"]
        return st_o
    n_o, pose_o, outl_o = oracle_mod.pose_optimization(*arrays, K_KITTI, C.BF)
    assert np.abs(got["pose"] - pose_o).max() < POSE_TOL
    assert got["stats"].tolist() == [n_o]
    assert np.array_equal(got["outlier"], outl_o)
    return None


@pytest.mark.parametrize("name", C.NAMES)
def test_solve_keeps_its_bits(ctx, oracle_mod, golden, monkeypatch, name):
    case = C.BY_NAME[name]
    arrays = C.inputs(case)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    got = C.solve(ctx, case, arrays)
    _check_golden(golden, case, arrays, got)
    st_o = _check_oracle(oracle_mod, case, arrays, got)
    if case["chain"]:
        # the candidate table is really used, and serves the bits of a solve per lambda
        assert st_o["clean_rejections"] >= 4 and st_o["max_reject_run"] >= 4, st_o
        monkeypatch.setenv("MMT_LM_MAX_CAND", "1")
        _check_golden(golden, case, arrays, C.solve(ctx, case, arrays))
