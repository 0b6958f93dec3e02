"""The CPU oracle's solves at an anisotropic camera (fx != fy), against ground truth and the
float64 edge models of tests/solve_ref_py.py.  No GPU: a mistake the oracle shares with the
product (the GPU tests compare the two) is found here.

  * consistent data (no noise, no outliers, float32 inputs): the returned pose within the
    project's bar (1e-4) of the true one -- after asserting that the float64 minimiser of the same
    inputs lies within 1e-5 of it, so that a miss belongs to the solver;
  * PnP with gross outliers: the ground-truth inlier set exactly, the pose within the bar;
  * PoseOptimization with noise and outliers: outlier flags equal to a float64 evaluation of each
    edge's chi2 at the returned pose, and the pose at the least-squares minimum of its inliers.
Every case also asserts that exchanging fx and fy changes the oracle's answer."""
import numpy as np
import pytest

import aniso_cases as A
import solve_ref_py as S
from camera_cases import BF_ANISO, K_ANISO, swap_fxfy

K, BF = K_ANISO, BF_ANISO
K_SWAP = swap_fxfy(K)


def _d(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


@pytest.mark.parametrize("seed,n,mono", A.POSE_CONSISTENT)
def test_pose_optimization_consistent(oracle_mod, seed, n, mono):
    Xw, obs, s2, init, T = A.pose_consistent(seed, n, mono)
    assert _d(S.gauss_newton_pose(S.pose_residual_fn(Xw, obs, s2, K, BF), init), T) < A.GN_TOL
    n_in, pose, outl = oracle_mod.pose_optimization(Xw, obs, s2, init, K, BF)
    assert _d(pose, T) < A.POSE_TOL
    assert n_in == n and not outl.any()
    assert _d(oracle_mod.pose_optimization(Xw, obs, s2, init, K_SWAP, BF)[1], pose) > 100 * A.POSE_TOL


@pytest.mark.parametrize("seed,n,ego", A.FLOW_CONSISTENT)
def test_flow_solve_consistent(oracle_mod, seed, n, ego):
    obs, flow, depth, Tl, init, T = A.flow_consistent(seed, n)
    assert _d(S.gauss_newton_pose(S.flow_residual_fn(obs, flow, depth, Tl, K), init), T) < A.GN_TOL
    args = A.EGO if ego else A.OBJ
    rc, pose, st = oracle_mod.flow_solve(obs, flow, depth, Tl, init, *args, K)
    assert rc == 0 and st["inliers"] == n
    assert _d(pose, T) < A.POSE_TOL
    # the flow edges back-project and project with the same camera, so a swap nearly cancels:
    # still ten times the bar
    assert _d(oracle_mod.flow_solve(obs, flow, depth, Tl, init, *args, K_SWAP)[1], pose) > 10 * A.POSE_TOL


@pytest.mark.parametrize("seed,n,out", A.PNP_CASES)
def test_pnp_ransac_recovers_inliers_and_pose(oracle_mod, seed, n, out):
    p3, p2, T, inl = A.pnp_case(seed, n, out)
    assert S.reprojection_sq_error(T, p3, p2, K)[inl].max() < 1e-5
    assert len(inl) == n or np.sqrt(np.delete(S.reprojection_sq_error(T, p3, p2, K), inl).min()) >= 20
    assert _d(S.gauss_newton_pose(S.reprojection_residual_fn(p3, p2, K, keep=inl), np.eye(4)), T) < A.GN_TOL
    rc, R, t, got, _ = oracle_mod.pnp_ransac(p3, p2, K)
    assert rc == 0
    assert sorted(got.tolist()) == inl.tolist()
    assert _d(R, T[:3, :3]) < A.POSE_TOL and _d(t, T[:3, 3]) < A.POSE_TOL
    assert len(oracle_mod.pnp_ransac(p3, p2, K_SWAP)[3]) < len(inl) // 2


@pytest.mark.parametrize("seed,n,out", A.P4P_CASES)
def test_pnpsolver_recovers_inliers_and_pose(oracle_mod, seed, n, out):
    p3, p2, s2, T, mask = A.p4p_case(seed, n, out)
    chi2 = S.reprojection_sq_error(T, p3, p2, K) / s2
    assert chi2[mask].max() < 1e-4 and (mask.all() or chi2[~mask].min() > 100)
    init = S.se3_exp([0.01, 0.0, -0.01, 0.05, 0.0, 0.1]) @ T.astype(np.float64)
    assert _d(S.gauss_newton_pose(S.reprojection_residual_fn(p3, p2, K, keep=mask), init), T) < A.GN_TOL
    randi = oracle_mod.p4p_randi(n, 400, seed + 1)
    r = oracle_mod.pnpsolver_iterate(p3, p2, s2, K, randi, 5, {}, A.PNP_PARAMS)
    assert r["found"] and r["n_inliers"] == mask.sum()
    assert np.array_equal(r["mask"], mask)
    assert _d(r["Tcw"], T) < A.POSE_TOL
    assert not oracle_mod.pnpsolver_iterate(p3, p2, s2, K_SWAP, randi, 5, {}, A.PNP_PARAMS)["found"]


def _ba_precondition(P, Tt, X):
    """Each optimised keyframe's float64 minimiser over its own edges, the points held at their
    true (float32) positions, from the perturbed initial pose."""
    for k in np.nonzero(P["fixed"] == 0)[0]:
        sel = P["kf"] == k
        if sel.sum() < 6:
            continue
        sub = dict(pt=P["pt"][sel], kf=np.zeros(sel.sum(), int), obs=P["obs"][sel])
        w = np.sqrt(P["s"][sel].astype(np.float64))[:, None]
        got = S.gauss_newton_pose(lambda T: S.ba_residuals(T[None], X, sub, K, BF)[0] * w, P["T"][k])
        assert _d(got, Tt[k]) < A.GN_TOL, k


@pytest.mark.parametrize("seed,kw", A.BA_CONSISTENT)
def test_local_ba_consistent(oracle_mod, seed, kw):
    """Poses and points within the bar of the truth.  The case differs from ba_problem's default
    in its initial points (exact, not perturbed): see aniso_cases.BA_CONSISTENT_KW for what the
    reference's step policy does to a distant point's depth otherwise."""
    P, Tt, X = A.ba_consistent(seed, kw)
    assert np.abs(S.ba_residuals(Tt, X, P, K, BF)[0]).max() < 5e-3
    _ba_precondition(P, Tt, X)
    assert _d(P["T"], Tt) > 30 * A.TOL  # the solve has something to do
    To, Xo, erase, st = oracle_mod.local_ba(P, K, BF)
    assert not erase.any()
    assert _d(To, Tt) < A.TOL
    assert _d(Xo, X) < A.TOL
    assert _d(oracle_mod.local_ba(P, K_SWAP, BF)[0], To) > 10 * A.TOL


@pytest.mark.parametrize("seed,n,out,mono,d_o", A.POSE_NOISY)
def test_pose_optimization_noisy_flags_and_minimum(oracle_mod, seed, n, out, mono, d_o):
    """The seeds of aniso_cases.POSE_NOISY keep at most 2 % of their edges within 1 % of a chi2
    threshold at the oracle's pose, and the table's d_o is the oracle's distance to T_min."""
    Xw, obs, s2, init, _ = A.pose_noisy(seed, n, out, mono)
    n_in, pose, outl = oracle_mod.pose_optimization(Xw, obs, s2, init, K, BF)
    want, near = S.pose_outlier_flags(pose, Xw, obs, s2, K, BF, A.NEAR_MARGIN)
    print("near-threshold edges", int(near.sum()), "of", n)
    assert near.sum() <= A.NEAR_CAP * n
    assert np.array_equal(outl[~near], want[~near])
    assert n_in == n - outl.sum() and 0.05 * n <= outl.sum() <= 0.4 * n
    T_min = S.gauss_newton_pose(S.pose_residual_fn(Xw, obs, s2, K, BF, keep=~outl), pose)
    d = _d(pose, T_min)
    print("d_o", d)
    assert d < A.POSE_TOL
    # the table's d_o is this measurement (float32 pose entries: a few 1e-7 of slack for another
    # compiler's rounding)
    assert abs(d - d_o) <= 0.5 * d_o + 5e-7
    # the case is sensitive: at the swapped camera the flags change
    outl_s = oracle_mod.pose_optimization(Xw, obs, s2, init, K_SWAP, BF)[2]
    assert (outl_s != outl).sum() > 0.1 * n
