"""The EPnP solvers and the object front end's stage B keep their bits through changes to
csrc/mmt_pnp.hip and k_obj_stage_b that are meant to leave the arithmetic alone (first of them: one
statement of each EPnP stage shared by the hypothesis and the refit kernels, one inlier-mask loop,
one compaction, the unfused stage-B kernels removed).  Every output of ctx.pnp_ransac (D5),
ctx.pnpsolver_iterate (D6) and, per frame and object, of stage B through ctx.track on the cases of
tests/pnp_bits_cases.py must equal, bit for bit, what the commit before that change computed
(tests/golden/pnp_golden.npz, recorded by tools/make_golden_pnp.py on that commit), and agree with
the CPU oracle as in test_gpu_track.py::test_pnp_ransac_matches_oracle, test_gpu_pnpsolver._compare
and oracle.compare.compare_frame, so a wrong golden cannot hide.

The cases are the smallest at which each path can go wrong: D5 at count == modelPoints (no
iterations), the smallest count that iterates, under one wave, the wave / mask-word boundary
(64 / 65), the second round of the 256-thread scoring loops (257), of every refit loop and of the
compaction (360 inliers of 513), and a failed RANSAC (identity Rt); D6 with Refine on the first
iteration, exhausted iterations, the word boundary, the second round of the refit loops and nothing
found; stage B with no motion model, a motion model that loses, one with no inliers, a failed
RANSAC, and ties (the motion model chosen).  test_oracle_takes_the_listed_paths needs no GPU."""
import os

import numpy as np
import pytest

import pnp_bits_cases as C
from synth_problems import K_KITTI

POSE_TOL = 1e-4    # test_gpu_track.py's and test_gpu_pnpsolver.py's
CENTRE_TOL = 1e-3  # test_gpu_track.py's
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pnp_golden.npz")


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


_ORACLE = {}


def oracle_result(oracle_mod, case):
    """The CPU oracle's result of a case, computed once and shared by the tests."""
    name = case["name"]
    if name in _ORACLE:
        return _ORACLE[name]
    arrays = C.inputs(case)
    if case["kind"] == "d5":
        r = oracle_mod.pnp_ransac(*arrays, K_KITTI)
    elif case["kind"] == "d6":
        st = {}
        r = (oracle_mod.pnpsolver_iterate(*arrays, K_KITTI, C.randi(oracle_mod, case),
                                          C.P4P_ITERATIONS, st, C.P4P_PARAMS), st)
    else:
        tr = oracle_mod.Tracker(1242, 375, K_KITTI, C.BF, 0, 2000)
        r = [tr.track(f["bgr"], f["disp"], f["flow"], f["sem"]) for f in arrays]
    _ORACLE[name] = r
    return r


def _check_golden(golden, case, arrays, draws, got):
    name = case["name"]
    assert str(golden[name + ".sha256"]) == C.input_digest(case, arrays, draws), \
        "%s: the generated problem differs from the one the golden was recorded on; record " \
        "again on the yardstick commit" % name
    for k, v in got.items():
        g = golden["%s.%s" % (name, k)]  # every output is held: none was unrepeatable
        assert v.dtype == g.dtype and v.shape == g.shape, (name, k, v.dtype, g.dtype)
        assert np.array_equal(v, g, equal_nan=True), (name, k, v, g)


def _check_oracle(case, raw, ref):
    if case["kind"] == "d5":  # test_gpu_track.py::test_pnp_ransac_matches_oracle
        R_g, t_g, inl_g, info_g = raw
        rc, R_o, t_o, inl_o, info_o = ref
        assert info_g["iterations"] == info_o["iterations"]
        assert info_g["best_iter"] == info_o["best_iter"]
        assert sorted(inl_g.tolist()) == sorted(inl_o.tolist())
        if rc == 0:
            assert np.abs(R_g - R_o).max() < POSE_TOL
            assert np.abs(t_g - t_o).max() < POSE_TOL
        else:
            assert np.array_equal(R_g, np.eye(3)) and not t_g.any()
    elif case["kind"] == "d6":  # test_gpu_pnpsolver._compare
        (g, gs), (o, os_) = raw, ref
        assert g["found"] == o["found"] and g["no_more"] == o["no_more"]
        assert g["n_inliers"] == o["n_inliers"]
        assert np.array_equal(g["mask"], o["mask"])
        assert gs["iterations"] == os_["iterations"] and gs["best_inliers"] == os_["best_inliers"]
        assert np.array_equal(gs["best_mask"], os_["best_mask"])
        if g["found"]:
            assert np.abs(g["Tcw"] - o["Tcw"]).max() < POSE_TOL
        if gs["best_inliers"]:
            assert np.abs(gs["best_Tcw"] - os_["best_Tcw"]).max() < POSE_TOL
    else:  # test_gpu_track._compare_frame
        from oracle import compare
        assert len(raw) == len(ref)
        for i, (g, o) in enumerate(zip(raw, ref)):
            p, c, bad = compare.compare_frame(g, o)[:3]
            assert not bad, (i, bad)
            assert p < POSE_TOL, (i, p)
            assert c < CENTRE_TOL, (i, c)


@pytest.mark.gpu
@pytest.mark.parametrize("name", C.NAMES)
def test_pnp_keeps_its_bits(ctx, oracle_mod, golden, name):
    case = C.BY_NAME[name]
    arrays = C.inputs(case)
    draws = C.randi(oracle_mod, case) if case["kind"] == "d6" else None
    raw, got = C.solve(ctx, case, arrays, draws)
    _check_golden(golden, case, arrays, draws, got)
    _check_oracle(case, raw, oracle_result(oracle_mod, case))


def _objects(frames):
    return [[(o["label"], o["ransac_inliers"], o["mm_inliers"], o["n_solve"]) for o in f["objects"]]
            for f in frames]


@pytest.mark.parametrize("name", C.NAMES)
def test_oracle_takes_the_listed_paths(oracle_mod, name):
    """The oracle alone, on any machine: each case exercises the path it is listed for."""
    case = C.BY_NAME[name]
    ref = oracle_result(oracle_mod, case)
    if case["kind"] == "d5":
        rc, R, t, inl, info = ref
        want = case["oracle"]
        assert len(inl) == want["inliers"] and rc == (0 if want["inliers"] else 1)
        for k in ("iterations", "best_iter"):
            if want[k] is not None:
                assert info[k] == want[k]
        if case["n"] > 5 and want["inliers"]:  # it iterates, and stops early
            assert 0 < info["iterations"] < 500 and 0 <= info["best_iter"] < info["iterations"]
        if not want["inliers"]:
            assert np.array_equal(R, np.eye(3)) and not t.any()
    elif case["kind"] == "d6":
        r, st = ref
        got = dict(r, iterations=st["iterations"])
        for k, v in case["oracle"].items():
            assert got[k] == v, (k, got[k], v)
        if r["found"] and not r["no_more"]:  # Refine() reached and returned
            assert r["n_inliers"] > 10
        if r["found"] and r["no_more"]:      # exhausted: the best hypothesis as it is
            assert r["n_inliers"] == st["best_inliers"] and np.array_equal(r["mask"], st["best_mask"])
    elif name == "track_kitti":
        objs = [o for f in _objects(ref) for o in f]
        # the motion model is evaluated with 4, 39 and 0 inliers and always loses to RANSAC
        assert [o[2] for o in objs] == [-1, 4, 39, 0]
        assert all(o[1] > o[2] and o[3] == o[1] for o in objs)
    else:
        fr = _objects(ref)
        assert fr[0] == [] and [[o[0] for o in f] for f in fr[1:]] == [[1, 2, 3]] * 5
        assert all(o[2] == -1 for o in fr[1])       # frame 1: no motion model
        assert fr[1][2][1] == 0 and fr[1][2][3] == 0  # object 3's RANSAC fails
        assert fr[2][2][2] == 0 and fr[2][2][1] > 0 and fr[2][2][3] == fr[2][2][1]  # RANSAC chosen
        ties = fr[2][:2] + [o for f in fr[3:] for o in f]
        assert len(ties) == 11 and all(o[1] == o[2] == o[3] > 0 for o in ties)  # motion model chosen
