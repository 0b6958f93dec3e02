"""Every camera-consuming GPU probe, and one short drive, at an anisotropic camera (fx != fy).

The rest of the suite runs with K_KITTI (fx == fy) or a uniform scaling of it, where a kernel
that read fx for fy would go unnoticed.  Here the camera is camera_cases.K_ANISO / BF_ANISO:

  a. the solves against the CPU oracle, with the comparisons and tolerances of test_gpu_track.py,
     test_gpu_pnpsolver.py and test_gpu_localmap.py;
  b. the solves against ground truth on consistent data and against the float64 edge models of
     tests/solve_ref_py.py (the cases test_oracle_aniso.py holds the oracle to on the CPU);
  c. the frame grid, the projection matchers, Fuse, SearchForTriangulation, SearchBySim3 and the
     Sim3Solver against the oracle / tests/sim3_ref_py.py, bit for bit;
  d. a 40-frame drive at 3/4 resolution with the vocabulary loaded and one textureless frame.

Each case asserts on the reference side that exchanging fx and fy changes the expected output
(for the frame grid, which reads bf alone: that another bf does)."""
import numpy as np
import pytest

import aniso_cases as A
import solve_ref_py as S
from ba_problems import ba_problem
from camera_cases import (BF_ANISO, BF_ANISO_34, K_ANISO, K_ANISO_34, K_ANISO_34_DICT, swap_fxfy)
from synth_problems import flow_problem, p4p_problem, pnp_problem, pose_opt_problem

pytestmark = pytest.mark.gpu
K, BF = K_ANISO, BF_ANISO
K_SWAP = swap_fxfy(K)
POSE_TOL, TOL = A.POSE_TOL, A.TOL
W, H = 1242, 375


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    cfg = M.kitti03_config(W, H, 2000, max_batch=8)
    cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.bf = K + (BF,)
    c = M.Context(cfg)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scale(oracle_mod):
    return np.asarray(oracle_mod.orb_config()["scale"], np.float32)


def _d(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


# ------------------------------------------------------------------ a. solves against the oracle
@pytest.mark.parametrize("seed,n,out,ego,groups", [
    (0, 64, 0.0, True, None), (1, 65, 0.1, False, None), (2, 400, 0.2, True, None),
    (3, 400, 0.15, False, None), (2, 400, 0.2, True, "3"), (6, 65, 0.3, True, "8"),
    (1, 64, 0.1, True, "2"), (1, 600, 0.1, True, None)])
def test_flow_solve_matches_oracle(ctx, oracle_mod, seed, n, out, ego, groups, monkeypatch):
    """Ego and object settings, whole and split (MMT_LM_SPLIT) solves, 64 / 65 / 400 edges (one
    and two edges a thread), and 600, which splits on its own."""
    if groups is not None:
        monkeypatch.setenv("MMT_LM_SPLIT", groups)
    obs, flow, depth, Tl, init, _ = flow_problem(seed, n, outlier_frac=out, K=K)
    args = A.EGO if ego else A.OBJ
    rc, pose_o, st_o = oracle_mod.flow_solve(obs, flow, depth, Tl, init, *args, K)
    assert _d(oracle_mod.flow_solve(obs, flow, depth, Tl, init, *args, K_SWAP)[1], pose_o) > POSE_TOL
    status, pose_g, st_g = ctx.flow_solve(obs, flow, depth, Tl, init, *args, K)
    assert status == rc == 0
    assert np.abs(pose_g - pose_o).max() < POSE_TOL
    assert st_g["inliers"] == st_o["inliers"]
    assert st_g["iterations"] == st_o["iterations"]


def test_flow_solve_rejection_chain(ctx, oracle_mod, monkeypatch):
    """A large motion without noise: trials rejected in a row on clean systems, so the lambda
    candidates solved in advance are used; bit-identical to solving every trial for its own
    lambda, and within the bar of the oracle."""
    obs, flow, depth, Tl, init, _ = flow_problem(3, 40, outlier_frac=0.0, pix_noise=0.0,
                                                 motion=0.3, K=K)
    rc, pose_o, st_o = oracle_mod.flow_solve(obs, flow, depth, Tl, init, *A.OBJ, K)
    assert st_o["clean_rejections"] >= 4 and st_o["max_reject_run"] >= 4, st_o
    assert _d(oracle_mod.flow_solve(obs, flow, depth, Tl, init, *A.OBJ, K_SWAP)[1], pose_o) > POSE_TOL
    status4, pose4, st4 = ctx.flow_solve(obs, flow, depth, Tl, init, *A.OBJ, K)
    monkeypatch.setenv("MMT_LM_MAX_CAND", "1")
    status1, pose1, st1 = ctx.flow_solve(obs, flow, depth, Tl, init, *A.OBJ, K)
    assert status4 == status1 == rc == 0
    assert np.array_equal(pose4, pose1) and st4 == st1
    assert np.abs(pose4 - pose_o).max() < POSE_TOL
    assert st4["inliers"] == st_o["inliers"]


@pytest.mark.parametrize("seed,n,out,mono", [(0, 40, 0.15, 0.0), (1, 40, 0.15, 0.2),
                                             (2, 40, 0.15, 1.0), (3, 300, 0.15, 0.0),
                                             (4, 300, 0.2, 0.2), (5, 300, 0.0, 1.0),
                                             (6, 1100, 0.1, 0.2), (7, 2049, 0.1, 0.1)])
def test_pose_optimization_matches_oracle(ctx, oracle_mod, seed, n, out, mono):
    """40 and 300 edges (two a thread), 1100 (four a thread) and 2049 (the scratch kernel, which
    has its own copy of the edge model)."""
    Xw, obs, s2, init, _ = pose_opt_problem(seed, n, outlier_frac=out, mono_frac=mono, K=K, bf=BF)
    n_o, pose_o, outl_o = oracle_mod.pose_optimization(Xw, obs, s2, init, K, BF)
    assert _d(oracle_mod.pose_optimization(Xw, obs, s2, init, K_SWAP, BF)[1], pose_o) > POSE_TOL
    n_g, pose_g, outl_g = ctx.pose_optimization(Xw, obs, s2, init, K, BF)
    assert np.abs(pose_g - pose_o).max() < POSE_TOL
    assert n_g == n_o
    assert np.array_equal(outl_g, outl_o)


@pytest.mark.parametrize("seed,n,out", [(0, 60, 0.3), (1, 400, 0.5)])
def test_pnp_ransac_matches_oracle(ctx, oracle_mod, seed, n, out):
    p3, p2, _ = pnp_problem(seed, n, outlier_frac=out, pix_noise=0.05, K=K)
    rc, R_o, t_o, inl_o, info_o = oracle_mod.pnp_ransac(p3, p2, K)
    assert rc == 0 and len(oracle_mod.pnp_ransac(p3, p2, K_SWAP)[3]) < len(inl_o) // 2
    R_g, t_g, inl_g, info_g = ctx.pnp_ransac(p3, p2, K)
    assert info_g["iterations"] == info_o["iterations"]
    assert info_g["best_iter"] == info_o["best_iter"]
    assert sorted(inl_g.tolist()) == sorted(inl_o.tolist())
    assert np.abs(R_g - R_o).max() < POSE_TOL
    assert np.abs(t_g - t_o).max() < POSE_TOL


@pytest.mark.parametrize("seed,n,out,noise", [(6, 15, 0.0, 0.5), (1, 200, 0.3, 0.3)])
def test_pnpsolver_matches_oracle(ctx, oracle_mod, seed, n, out, noise):
    from test_gpu_pnpsolver import _compare
    p3, p2, s2, _ = p4p_problem(seed, n, outlier_frac=out, pix_noise=noise, K=K)
    randi = oracle_mod.p4p_randi(n, 400, seed + 1)
    gs, os_ = {}, {}
    o = oracle_mod.pnpsolver_iterate(p3, p2, s2, K, randi, 5, os_, A.PNP_PARAMS)
    swapped = oracle_mod.pnpsolver_iterate(p3, p2, s2, K_SWAP, randi, 5, {}, A.PNP_PARAMS)
    assert o["found"] and not np.array_equal(swapped["mask"], o["mask"])
    g = ctx.pnpsolver_iterate(p3, p2, s2, K, randi, 5, gs, A.PNP_PARAMS)
    _compare(g, o, gs, os_)


@pytest.mark.parametrize("seed,kw", [
    (12, dict(n_kf=4, n_fixed=1, n_pt=300, mono_frac=0.6, outlier_frac=0.1)),  # a small graph
    (31, dict(n_kf=6, n_fixed=2, n_pt=257, obs_per_pt=(1, 4))),  # one point past a point workgroup
    (31, dict(n_kf=6, n_fixed=2, n_pt=64, obs_per_pt=(1, 2))),   # no heavy point (> 2 edges)
])
def test_local_ba_matches_oracle(ctx, oracle_mod, seed, kw):
    P, _, _ = ba_problem(seed, K=K, bf=BF, **kw)
    if kw["n_pt"] == 64:
        assert np.bincount(P["pt"]).max() <= 2
    To, Xo, eo, so = oracle_mod.local_ba(P, K, BF)
    assert _d(oracle_mod.local_ba(P, K_SWAP, BF)[0], To) > TOL
    Tg, Xg, eg, sg = ctx.local_bundle_adjustment(P)
    assert sg == so, (sg, so)
    assert np.array_equal(eg, eo), (np.nonzero(eg != eo)[0][:10], eg.sum(), eo.sum())
    assert np.abs(Tg - To).max() < TOL
    assert np.abs(Xg - Xo).max() < TOL


# ------------------------------------------- b. solves against ground truth and the edge models
@pytest.mark.parametrize("seed,n,mono", A.POSE_CONSISTENT)
def test_pose_optimization_consistent(ctx, seed, n, mono):
    Xw, obs, s2, init, T = A.pose_consistent(seed, n, mono)
    assert _d(S.gauss_newton_pose(S.pose_residual_fn(Xw, obs, s2, K, BF), init), T) < A.GN_TOL
    n_in, pose, outl = ctx.pose_optimization(Xw, obs, s2, init, K, BF)
    assert _d(pose, T) < POSE_TOL
    assert n_in == n and not outl.any()


@pytest.mark.parametrize("seed,n,ego", A.FLOW_CONSISTENT)
def test_flow_solve_consistent(ctx, seed, n, ego):
    obs, flow, depth, Tl, init, T = A.flow_consistent(seed, n)
    assert _d(S.gauss_newton_pose(S.flow_residual_fn(obs, flow, depth, Tl, K), init), T) < A.GN_TOL
    status, pose, st = ctx.flow_solve(obs, flow, depth, Tl, init, *(A.EGO if ego else A.OBJ), K)
    assert status == 0 and st["inliers"] == n
    assert _d(pose, T) < POSE_TOL


@pytest.mark.parametrize("seed,kw", A.BA_CONSISTENT)
def test_local_ba_consistent(ctx, seed, kw):
    from test_oracle_aniso import _ba_precondition
    P, Tt, X = A.ba_consistent(seed, kw)
    _ba_precondition(P, Tt, X)
    Tg, Xg, erase, _ = ctx.local_bundle_adjustment(P)
    assert not erase.any()
    assert _d(Tg, Tt) < TOL
    assert _d(Xg, X) < TOL


@pytest.mark.parametrize("seed,n,out,mono,d_o", A.POSE_NOISY)
def test_pose_optimization_noisy_flags_and_minimum(ctx, seed, n, out, mono, d_o):
    """mvbOutlier equals a float64 evaluation of every edge's chi2 at the returned pose (edges
    within 1 % of a threshold excluded, at most 2 % of them), and the pose lies at the float64
    least-squares minimum of the returned inliers, within max(1e-4, 2 d_o) where d_o is the
    oracle's own distance to that minimum (aniso_cases.POSE_NOISY)."""
    Xw, obs, s2, init, _ = A.pose_noisy(seed, n, out, mono)
    n_in, pose, outl = ctx.pose_optimization(Xw, obs, s2, init, K, BF)
    want, near = S.pose_outlier_flags(pose, Xw, obs, s2, K, BF, A.NEAR_MARGIN)
    assert near.sum() <= A.NEAR_CAP * n
    assert np.array_equal(outl[~near], want[~near])
    assert n_in == n - outl.sum()
    T_min = S.gauss_newton_pose(S.pose_residual_fn(Xw, obs, s2, K, BF, keep=~outl), pose)
    d = _d(pose, T_min)
    print("distance to T_min", d, "d_o", d_o)
    assert d < max(POSE_TOL, 2 * d_o)


@pytest.mark.parametrize("seed,n,out", A.PNP_CASES)
def test_pnp_ransac_recovers_inliers_and_pose(ctx, seed, n, out):
    p3, p2, T, inl = A.pnp_case(seed, n, out)
    R, t, got, _ = ctx.pnp_ransac(p3, p2, K)
    assert sorted(got.tolist()) == inl.tolist()
    assert _d(R, T[:3, :3]) < POSE_TOL and _d(t, T[:3, 3]) < POSE_TOL


@pytest.mark.parametrize("seed,n,out", A.P4P_CASES)
def test_pnpsolver_recovers_inliers_and_pose(ctx, oracle_mod, seed, n, out):
    p3, p2, s2, T, mask = A.p4p_case(seed, n, out)
    randi = oracle_mod.p4p_randi(n, 400, seed + 1)  # glibc rand() draws, no solver code
    r = ctx.pnpsolver_iterate(p3, p2, s2, K, randi, 5, {}, A.PNP_PARAMS)
    assert r["found"] and r["n_inliers"] == mask.sum()
    assert np.array_equal(r["mask"], mask)
    assert _d(r["Tcw"], T) < POSE_TOL


# ------------------------------------------------------------------- c. matchers and geometry
def test_frame_grid(ctx, oracle_mod):
    """Frame::ComputeStereoFromRGBD reads bf alone (uR = u - bf / depth) and the grid no camera
    value at all: the sensitivity asserted is to bf."""
    import match_problems as MP
    k, _, dep = MP.frame(oracle_mod, 0)
    o = oracle_mod.frame_stereo_grid(k, dep, K, BF)
    assert not np.array_equal(o[0], oracle_mod.frame_stereo_grid(k, dep, K, MP.BF)[0])
    g = ctx.frame_grid(k, dep)
    for a, b in zip(g, o):
        assert np.array_equal(a, b)


def test_search_by_projection_frame(ctx, oracle_mod, scale):
    import match_problems as MP
    c = MP.sbp_case(oracle_mod, "forward", K=K)
    args = (c["kps"], c["desc"], c["depth"], c["tcw"], c["last_kps"], c["Xw"], c["mp_desc"],
            c["active"], c["tlw"], c["th"])
    onm, omatch = oracle_mod.search_by_projection_frame(*args, K, BF, scale, c["mono"],
                                                        c["check_orientation"], obs=c["obs"])
    snm, smatch = oracle_mod.search_by_projection_frame(*args, K_SWAP, BF, scale, c["mono"],
                                                        c["check_orientation"], obs=c["obs"])
    assert onm > 200 and (smatch != omatch).sum() > 50
    nm, match = ctx.search_by_projection_frame(*args, mono=c["mono"],
                                               check_orientation=c["check_orientation"],
                                               obs=c["obs"])
    assert nm == onm
    assert np.array_equal(match, omatch), np.nonzero(match != omatch)[0][:10]


def _local_args(oracle_mod):
    import match_problems as MP
    c = MP.local_case(oracle_mod, "rgbd", K=K)
    return c, (c["kps"], c["desc"], c["depth"], c["tcw"], c["Xw"], c["normal"], c["min_dist"],
               c["max_dist"], c["pdesc"], c["skip"], c["th"])


def test_search_local_points(ctx, oracle_mod, scale):
    c, args = _local_args(oracle_mod)
    onm, omatch, ofrus = oracle_mod.search_local_points(*args, K, BF, scale, c["taken"])
    snm, smatch, sfrus = oracle_mod.search_local_points(*args, K_SWAP, BF, scale, c["taken"])
    assert onm > 200 and (smatch != omatch).sum() > 50 and not np.array_equal(sfrus, ofrus)
    nm, match, frus = ctx.search_local_points(*args, taken=c["taken"])
    assert np.array_equal(frus, ofrus)
    assert nm == onm
    assert np.array_equal(match, omatch), np.nonzero(match != omatch)[0][:10]


def test_fuse_candidates(ctx, oracle_mod):
    """Fuse's search over the local-points case: the projection window from fx, fy, and the
    stereo reprojection gate from bf."""
    _, args = _local_args(oracle_mod)
    a = args[:9]
    io, do = oracle_mod.fuse_candidates(*a, K, BF, W, H)
    assert (io >= 0).sum() > 200
    assert (oracle_mod.fuse_candidates(*a, K_SWAP, BF, W, H)[0] != io).sum() > 50
    assert (oracle_mod.fuse_candidates(*a, K, 1.2 * BF, W, H)[0] != io).sum() > 0
    ig, dg = ctx.fuse_candidates(*a)
    assert np.array_equal(ig, io) and np.array_equal(dg, do)


def test_search_by_projection_keyframe(ctx, oracle_mod, scale):
    import reloc_problems as RP
    c = RP.sbp_case(oracle_mod, "round1", K=K)
    nm_o, m_o = oracle_mod.search_by_projection_keyframe(*RP.sbp_args(c), K, BF, scale)
    nm_s, m_s = oracle_mod.search_by_projection_keyframe(*RP.sbp_args(c), K_SWAP, BF, scale)
    assert nm_o > 200 and (m_s != m_o).sum() > 50
    nm_g, m_g, _ = ctx.search_by_projection_keyframe(*RP.sbp_args(c))
    assert np.array_equal(m_g, m_o), np.nonzero(m_g != m_o)[0][:10]
    assert nm_g == nm_o


def test_search_for_triangulation(ctx, oracle_mod, scale):
    """ComputeF12 = K^-T [t12]x R12 K^-1 and the epipolar test on it: F12 bit for bit."""
    import reloc_problems as RP
    c = RP.sft_case(oracle_mod, "kitti", K=K, BF=BF)
    nm_o, m_o, F_o = oracle_mod.search_for_triangulation(c["kf1"], c["kf2s"], K, BF, scale)
    nm_s, m_s, F_s = oracle_mod.search_for_triangulation(c["kf1"], c["kf2s"], K_SWAP, BF, scale)
    assert nm_o.min() > 30 and not np.array_equal(F_s, F_o) and not np.array_equal(m_s, m_o)
    nm_g, m_g, F_g = ctx.search_for_triangulation(c["kf1"], c["kf2s"])
    assert np.array_equal(F_g.view(np.uint32), F_o.view(np.uint32)), (F_g, F_o)
    assert np.array_equal(m_g, m_o), np.argwhere(m_g != m_o)[:10]
    assert np.array_equal(nm_g, nm_o)


def test_search_by_sim3(ctx):
    import sim3_cases as SC
    import sim3_ref_py as R
    s, _ = SC.orb_scales()
    kf1, kf2, sim3, pair = SC.keyframe_pair(11, 220, s12=1.15, K=K)
    none = np.full(len(kf1["skip"]), -1, np.int32)
    a = (kf1, kf2, sim3["s"], sim3["R"], sim3["t"], 7.5, none)
    ref = R.search_by_sim3(*a, K, SC.W, SC.H, s)
    assert np.array_equal(ref["match"][:len(pair)], pair) and ref["n_found"] == len(pair)
    assert R.search_by_sim3(*a, K_SWAP, SC.W, SC.H, s)["n_found"] < len(pair) // 2
    nf, match, c1, c2 = ctx.search_by_sim3(*a)
    assert np.array_equal(c1, ref["cand1"]) and np.array_equal(c2, ref["cand2"])
    assert np.array_equal(match, ref["match"]) and nf == ref["n_found"]


K2_ANISO = (700.0, 640.0, 620.0, 190.0)  # the second keyframe's camera in the Sim3Solver cases


@pytest.mark.parametrize("n,out,noise,fix,seed", [(257, 0.4, 2.0, True, 50),
                                                  (120, 0.3, 2.0, False, 49)])
def test_sim3solver(ctx, n, out, noise, fix, seed):
    """Two different anisotropic cameras.  The solver projects a point and its observation with
    the same camera, so an inlier stays one under any camera; the camera acts on the points near
    a threshold (noise of 2 px), and exchanging fx and fy of either camera changes the mask."""
    import sim3_cases as SC
    import sim3_ref_py as R
    from test_gpu_sim3solver import assert_clear_of_thresholds, compare, ref_solver
    p = SC.solver_problem(seed, n, out, noise, fix, K1=K, K2=K2_ANISO)
    randi = SC.draws(seed + 100, n, 320)
    ref = ref_solver(p)
    o = ref.iterate(5, randi)
    assert_clear_of_thresholds(ref)
    assert o["found"]
    for k1, k2 in ((K_SWAP, K2_ANISO), (K, swap_fxfy(K2_ANISO))):
        other = ref_solver(dict(p, K1=k1, K2=k2)).iterate(5, randi)
        assert not np.array_equal(other["mask"], o["mask"])
    gs = {}
    g = ctx.sim3solver_iterate([p], [randi], 5, [gs])[0]
    compare(g, gs, o, ref)


# --------------------------------------------------------------------------------- d. one drive
DRIVE_LOST = 24  # the textureless frame


def test_vocabulary_drive_three_quarter_res(oracle_mod):
    """test_gpu_vocab.py's 3/4-resolution drive at the 3/4 variant of K_ANISO: 931x281, 1000
    features, 40 frames, the vocabulary loaded, one textureless frame.  Frame by frame within the
    bar of the oracle, vocabulary counters and the final map graph equal, and the
    TrackReferenceKeyFrame / Relocalization / SearchByProjection(F, KF) / CreateNewMapPoints
    paths all taken."""
    from oracle import compare
    from test_gpu_vocab import BOW_KEYS, _check_maps, _run_pair
    assert K_ANISO_34[0] != K_ANISO_34[1]
    got, ora, gb, ob, gm, om = _run_pair(oracle_mod, 931, 281, K_ANISO_34_DICT, BF_ANISO_34, 1000,
                                         40, [DRIVE_LOST])
    rec = compare.parity_record(got, ora)
    print("parity", rec, "\nbow counters", ob, "\nmap states", [o["map_state"] for o in ora])
    assert rec["first_divergent_frame"] is None, rec
    assert {k: gb[k] for k in BOW_KEYS} == {k: ob[k] for k in BOW_KEYS}
    assert ob["trk_ok"] >= 1 and ob["reloc"] >= 1 and ob["triangulated"] > 0
    assert ob["sbp_rounds"] >= 1 and ob["reloc_ok"] >= 1
    _check_maps(gm, om)

