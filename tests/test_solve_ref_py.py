"""Pins tests/solve_ref_py.py (the float64 edge models the anisotropic-camera tests check the
solves against) on facts that do not depend on it: residuals vanish at the true pose of data
built with synth_problems.project (written separately), hand-computed edges at fx != fy give
their known chi2, exchanging fx and fy changes every result, and gauss_newton_pose finds the true
pose from the perturbed initial estimates of the synthetic problems.  CPU only."""
import numpy as np
import pytest

import solve_ref_py as S
from ba_problems import ba_problem
from camera_cases import BF_ANISO, K_ANISO, swap_fxfy
from synth_problems import flow_problem, p4p_problem, pose_opt_problem, project, rot, se3

K_SWAP = swap_fxfy(K_ANISO)


def _pose(seed):
    rng = np.random.default_rng(seed)
    return se3(rot(rng.normal(size=3), 0.2 * rng.normal()), rng.normal(size=3)).astype(np.float64)


def _cloud(seed, n, T, K):
    """n world points in front of camera T, float64, and their exact pixels / depths."""
    rng = np.random.default_rng(seed + 100)
    pc = np.stack([rng.uniform(-8, 8, n), rng.uniform(-2, 2, n), rng.uniform(4, 40, n)], 1)
    Ti = np.linalg.inv(T)
    Xw = pc @ Ti[:3, :3].T + Ti[:3, 3]
    uv, z = project(T, Xw, K)
    return Xw, uv, z


def test_hand_computed_edges():
    """R = 90 degrees about z, t = (4, 0, 2), Xw = (1, 2, 8): the camera point is (2, 1, 10), so
    u = 0.2 fx + cx = 745.55754, v = 0.1 fy + cy = 249.025, uR = u - 352 / 10 = 710.35754.
    Mono observation (u + 1, v - 2): e = (1, -2), chi2 = 5 * 0.25.  Stereo observation
    (u + 1, v - 2, uR + 0.5): e = (1, -2, 0.5), chi2 = 5.25 * 0.25."""
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [4, 0, 2]
    Xw = np.array([[1.0, 2.0, 8.0]] * 2)
    u, v, ur = 0.2 * 721.5377 + 601.25, 0.1 * 655.25 + 183.5, 0.2 * 721.5377 + 601.25 - 35.2
    assert abs(u - 745.55754) < 1e-9 and abs(v - 249.025) < 1e-9 and abs(ur - 710.35754) < 1e-9
    obs = np.array([[u + 1, v - 2, -1.0], [u + 1, v - 2, ur + 0.5]])
    e, mono = S.pose_edge_errors(T, Xw, obs, K_ANISO, BF_ANISO)
    assert mono.tolist() == [True, False]
    assert np.allclose(e, [[1, -2, 0], [1, -2, 0.5]], atol=1e-10)
    chi2 = S.chi2_pose_edges(T, Xw, obs, [0.25, 0.25], K_ANISO, BF_ANISO)
    assert np.allclose(chi2, [1.25, 1.3125], atol=1e-10)
    # the BA edges are the same errors with the point a vertex
    eb, _ = S.ba_residuals(T[None], Xw[:1], dict(pt=[0, 0], kf=[0, 0], obs=obs), K_ANISO, BF_ANISO)
    assert np.allclose(eb, e, atol=1e-10)
    assert np.allclose(S.reprojection_sq_error(T, Xw, obs[:, :2], K_ANISO), [5, 5], atol=1e-9)
    # fy read as fx moves v by 0.1 * (fx - fy) = 6.62877
    es, _ = S.pose_edge_errors(T, Xw, obs, K_SWAP, BF_ANISO)
    assert np.allclose(es[:, 1] - e[:, 1], -0.1 * (721.5377 - 655.25), atol=1e-9)
    flags, near = S.pose_outlier_flags(T, Xw, obs * [1, 1, 1], [0.25, 0.25], K_ANISO, BF_ANISO, 0.01)
    assert not flags.any() and not near.any()


def test_hand_computed_flow_edge():
    """Last camera at the identity, current camera translated by (0.5, 0, -1): the pixel
    (cx + 100, cy + 50) at depth 10 is the point (100 * 10 / fx, 50 * 10 / fy, 10); in the current
    camera z = 9, so p = (fx (x + 0.5) / 9 + cx, fy y / 9 + cy) = (cx + (1000 + 0.5 fx) / 9,
    cy + 500 / 9).  With the flow vertex at (3, 4) the projection error is
    (100 + 3 - (1000 + 0.5 fx) / 9, 50 + 4 - 500 / 9); the prior error against a measured flow of
    (1, 1) is (2, 3)."""
    fx, fy, cx, cy = K_ANISO
    T = np.eye(4)
    T[:3, 3] = [0.5, 0, -1]
    obs = np.array([[cx + 100, cy + 50]])
    ep, eq = S.flow_residuals(T, [[3.0, 4.0]], obs, [[1.0, 1.0]], [10.0], np.eye(4), K_ANISO)
    want = [103 - (1000 + 0.5 * fx) / 9, 54 - 500 / 9]
    assert np.allclose(ep, [want], atol=1e-9) and np.allclose(eq, [[2, 3]], atol=1e-12)
    c_p, c_q = S.flow_chi2(T, [[3.0, 4.0]], obs, [[1.0, 1.0]], [10.0], np.eye(4), K_ANISO, 0.3)
    assert np.allclose(c_p, 0.1 * (want[0] ** 2 + want[1] ** 2)) and np.allclose(c_q, 0.3 * 13)


def test_residuals_vanish_on_exact_data():
    T = _pose(1)
    Xw, uv, z = _cloud(1, 50, T, K_ANISO)
    obs = np.concatenate([uv, (uv[:, 0] - BF_ANISO / z)[:, None]], 1)
    obs[::3, 2] = -1.0
    s = np.full(50, 0.5)
    assert S.chi2_pose_edges(T, Xw, obs, s, K_ANISO, BF_ANISO).max() < 1e-16
    assert S.reprojection_sq_error(T, Xw, uv, K_ANISO).max() < 1e-16
    # the swapped camera does not explain the data: the case is sensitive to fx vs fy
    assert np.median(S.chi2_pose_edges(T, Xw, obs, s, K_SWAP, BF_ANISO)) > 1.0
    assert np.median(S.reprojection_sq_error(T, Xw, uv, K_SWAP)) > 1.0
    # flow: the same cloud seen from a last and a current camera
    Tl = _pose(2)
    Xw, uvl, zl = _cloud(2, 50, Tl, K_ANISO)
    uvc, _ = project(T, Xw, K_ANISO)
    flow = uvc - uvl
    ep, eq = S.flow_residuals(T, flow, uvl, flow, zl, Tl, K_ANISO)
    assert np.abs(ep).max() < 1e-8 and np.abs(eq).max() == 0
    eps, _ = S.flow_residuals(T, flow, uvl, flow, zl, Tl, K_SWAP)
    assert np.median(np.abs(eps)) > 0.5


@pytest.mark.parametrize("seed", [0, 1])
def test_residuals_vanish_on_float32_problems(seed):
    """The builders the solve tests use, without noise or outliers, at K_ANISO: at the true pose
    every residual is float32 rounding of the inputs (a few 1e-4 px)."""
    Xw, obs, s2, _, T = pose_opt_problem(seed, 80, outlier_frac=0, pix_noise=0, K=K_ANISO,
                                         bf=BF_ANISO)
    e, _ = S.pose_edge_errors(T, Xw, obs, K_ANISO, BF_ANISO)
    assert np.abs(e).max() < 2e-3
    assert np.median(np.abs(S.pose_edge_errors(T, Xw, obs, K_SWAP, BF_ANISO)[0][:, 1])) > 0.5
    o, f, d, Tl, _, Tc = flow_problem(seed, 80, outlier_frac=0, pix_noise=0, K=K_ANISO)
    ep, _ = S.flow_residuals(Tc, f, o, f, d, Tl, K_ANISO)
    assert np.abs(ep).max() < 2e-3
    # back-projection and projection with the same wrong camera cancel for a small motion: the
    # flow edges are the least sensitive, still ten times the rounding bound above
    assert np.median(np.abs(S.flow_residuals(Tc, f, o, f, d, Tl, K_SWAP)[0])) > 0.02
    p3, p2, _, Tp = p4p_problem(seed, 80, outlier_frac=0, pix_noise=0, K=K_ANISO)
    assert S.reprojection_sq_error(Tp, p3, p2, K_ANISO).max() < 4e-6
    P, Tt, X = ba_problem(seed, n_kf=4, n_fixed=1, n_pt=100, pix_noise=0, outlier_frac=0,
                          K=K_ANISO, bf=BF_ANISO)
    eb, _ = S.ba_residuals(Tt, X, P, K_ANISO, BF_ANISO)
    assert np.abs(eb).max() < 5e-3
    assert np.median(np.abs(S.ba_residuals(Tt, X, P, K_SWAP, BF_ANISO)[0][:, 1])) > 0.5


def test_se3_exp_is_a_rigid_motion():
    xi = np.array([0.3, -0.2, 0.5, 1.0, 2.0, -0.5])
    T = S.se3_exp(xi)
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-14)
    assert abs(np.linalg.det(T[:3, :3]) - 1) < 1e-14
    assert np.allclose(S.se3_exp(xi) @ S.se3_exp(-xi), np.eye(4), atol=1e-14)
    # pure rotation about z by pi / 2, and the small-angle branch
    Rz = S.se3_exp([0, 0, np.pi / 2, 0, 0, 0])
    assert np.allclose(Rz[:3, :3], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    assert np.allclose(S.se3_exp([1e-12, 0, 0, 1, 2, 3])[:3, 3], [1, 2, 3], atol=1e-11)


@pytest.mark.parametrize("seed,mono", [(0, 0.2), (1, 1.0), (2, 0.0)])
def test_gauss_newton_recovers_true_pose(seed, mono):
    """From pose_opt_problem's perturbed initial estimate (about 0.1 m, 0.02 rad off): exact
    float64 data to 1e-9, the float32 problem to 1e-5."""
    T = _pose(seed + 5)
    Xw, uv, z = _cloud(seed, 60, T, K_ANISO)
    obs = np.concatenate([uv, (uv[:, 0] - BF_ANISO / z)[:, None]], 1)
    obs[np.random.default_rng(seed).uniform(size=60) < mono, 2] = -1.0
    init = S.se3_exp([0.01, -0.02, 0.015, 0.1, -0.05, 0.08]) @ T
    got = S.gauss_newton_pose(S.pose_residual_fn(Xw, obs, np.ones(60), K_ANISO, BF_ANISO), init)
    assert np.abs(got - T).max() < 1e-9
    # the wrong camera has its minimum elsewhere
    bad = S.gauss_newton_pose(S.pose_residual_fn(Xw, obs, np.ones(60), K_SWAP, BF_ANISO), init)
    assert np.abs(bad - T).max() > 1e-3
    Xw, obs, s2, init, T = pose_opt_problem(seed, 120, outlier_frac=0, pix_noise=0, mono_frac=mono,
                                            K=K_ANISO, bf=BF_ANISO)
    got = S.gauss_newton_pose(S.pose_residual_fn(Xw, obs, s2, K_ANISO, BF_ANISO), init)
    assert np.abs(got - T).max() < 1e-5


def test_gauss_newton_on_flow_and_reprojection():
    o, f, d, Tl, init, Tc = flow_problem(3, 120, outlier_frac=0, pix_noise=0, K=K_ANISO)
    got = S.gauss_newton_pose(S.flow_residual_fn(o, f, d, Tl, K_ANISO), init)
    assert np.abs(got - Tc).max() < 1e-5
    p3, p2, _, T = p4p_problem(3, 120, outlier_frac=0, pix_noise=0, K=K_ANISO)
    got = S.gauss_newton_pose(S.reprojection_residual_fn(p3, p2, K_ANISO),
                              S.se3_exp([0.01, 0.0, -0.01, 0.05, 0.0, 0.1]) @ T)
    assert np.abs(got - T).max() < 1e-5
