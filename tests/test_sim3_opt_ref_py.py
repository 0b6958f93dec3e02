"""The NumPy restatement of Optimizer::OptimizeSim3 (tests/sim3_opt_ref_py.py) pinned to facts that
do not depend on it: closed forms of the Sim3 exponential, the group laws, an analytic Jacobian
written here, Huber values worked by hand, recovery of a known similarity, and the call's
bookkeeping (cleared pairs, the 10-pair rule, iteration caps, the first lambda of a round)."""
import math

import numpy as np
import pytest

import sim3_cases as C
import sim3_opt_cases as OC
import sim3_opt_ref_py as R
from camera_cases import K_ANISO

TOL = 1e-4


def rodrigues(w):
    th = np.linalg.norm(w)
    k = np.asarray(w) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def test_exp_pure_rotation_is_rodrigues():
    w = np.array([0.3, -0.2, 0.5])
    S = R.Sim3.exp([*w, 0, 0, 0, 0])
    assert S.branch == 1 and S.s == 1.0 and np.all(S.t == 0)
    assert np.allclose(S.R(), rodrigues(w), rtol=0, atol=1e-14)


def test_exp_pure_scale():
    ups, sigma = np.array([0.4, -1.1, 2.0]), 0.3
    S = R.Sim3.exp([0, 0, 0, *ups, sigma])
    s = math.exp(sigma)
    assert S.branch == 2 and S.s == s
    assert np.allclose(S.R(), np.eye(3), rtol=0, atol=1e-15)
    assert np.allclose(S.t, (s - 1) / sigma * ups, rtol=1e-14, atol=0)


@pytest.mark.parametrize("omega,sigma,branch", [((1e-7, 0, 0), 1e-7, 0), ((0.2, 0.1, 0), 1e-7, 1),
                                                 ((1e-7, 0, 0), 0.2, 2), ((0.2, 0.1, 0), 0.2, 3)])
def test_exp_takes_all_four_branches(omega, sigma, branch):
    """Both sides of eps = 1e-5 in sigma and in theta; each branch agrees with the matrix
    exponential of the generator [[sigma I + Omega, upsilon], [0, 0]] summed as a series.  The
    branch for both arguments large is exact; the other three drop the terms of first order in the
    small argument (1e-7 here), so they agree to 1e-6."""
    ups = np.array([0.3, -0.4, 0.5])
    S = R.Sim3.exp([*omega, *ups, sigma])
    assert S.branch == branch
    # the 4 x 4 generator: [[sigma I + Omega, upsilon], [0, 0]]
    G = np.zeros((4, 4))
    G[:3, :3] = sigma * np.eye(3) + R.skew(omega)
    G[:3, 3] = ups
    E, term = np.eye(4), np.eye(4)
    for k in range(1, 30):
        term = term @ G / k
        E = E + term
    atol = 1e-12 if branch == 3 else 1e-6
    assert np.allclose(S.s * S.R(), E[:3, :3], rtol=0, atol=atol)
    assert np.allclose(S.t, E[:3, 3], rtol=0, atol=atol)


def test_product_with_inverse_is_identity():
    rng = np.random.default_rng(3)
    S = R.Sim3.from_R(C.rot(rng.normal(size=3), 0.7), rng.normal(size=3), 1.3)
    for I in (S * S.inverse(), S.inverse() * S):
        assert abs(I.s - 1) < 1e-15
        assert np.allclose(I.R(), np.eye(3), rtol=0, atol=1e-15)
        assert np.allclose(I.t, 0, rtol=0, atol=1e-15)
    X = rng.normal(size=(5, 3))
    assert np.allclose(S.inverse().map(S.map(X)), X, rtol=0, atol=1e-14)


def analytic_jacobians(S, pr, fix_scale):
    """d e / d update for S' = exp(update) S.  With p = S X2: dp = omega x p + upsilon + sigma p, so
    J12 = -dpi(p) [-[p]x | I | p].  With p' = S^-1 X1 and S'^-1 = S^-1 exp(-update):
    dp' = -(1/s) R^T (omega x X1 + upsilon + sigma X1), so J21 = dpi(p') (1/s) R^T [-[X1]x | I | X1]."""
    def dpi(p, K):
        x, y, z = p
        return np.array([[K[0] / z, 0, -K[0] * x / z ** 2], [0, K[1] / z, -K[1] * y / z ** 2]])

    def gen(p):
        return np.concatenate([-R.skew(p), np.eye(3), p[:, None]], 1)

    n = len(pr["X1c"])
    J12, J21 = np.zeros((n, 2, 7)), np.zeros((n, 2, 7))
    Rm = S.R()
    for i in range(n):
        p = S.s * Rm @ pr["X2c"][i] + S.t
        J12[i] = -dpi(p, pr["K1"]) @ gen(p)
        X1 = pr["X1c"][i]
        q = Rm.T @ (X1 - S.t) / S.s
        J21[i] = dpi(q, pr["K2"]) @ (Rm.T / S.s) @ gen(X1)
    if fix_scale:
        J12[:, :, 6] = 0
        J21[:, :, 6] = 0
    return J12, J21


@pytest.mark.parametrize("fix_scale", [False, True])
def test_numeric_jacobian_against_analytic(fix_scale):
    """A central difference at h = 1e-9 in double: the truncation term h^2 f''' / 6 is below 1e-15
    relative.  What remains is rounding: an error is a difference of pixel coordinates up to 2^11,
    whose ulp is 4.5e-13; a handful of roundings per evaluation give about 1e-12 per error, so
    (e+ - e-) / 2e-9 carries up to about 1e-12 / 2e-9 = 5e-4 in absolute terms.  A row's largest
    entry is a rotation entry, f (1 + x^2 / z^2) for e12 and the same over the depth ratio for e21:
    about a focal length, 600 at the least here (asserted).  5e-4 is below 1e-6 of that; 1e-5 of
    it leaves a decade."""
    p = OC.problem(11, 40, fix_scale=fix_scale, K2=K_ANISO)
    pr = R.problem_arrays(p)
    S = R.Sim3.from_R(np.asarray(p["R12"], np.float64), np.asarray(p["t12"], np.float64),
                      float(p["s12"]))
    N12, N21 = R.numeric_jacobians(S, pr, fix_scale)
    A12, A21 = analytic_jacobians(S, pr, fix_scale)
    for N, A in ((N12, A12), (N21, A21)):
        scale = np.abs(A).max(axis=2, keepdims=True)
        assert scale.min() >= 600
        assert np.all(np.abs(N - A) <= 1e-5 * scale), float((np.abs(N - A) / scale).max())
    if fix_scale:
        assert np.all(N12[:, :, 6] == 0) and np.all(N21[:, :, 6] == 0)
    else:
        # a scale step from the left scales S X2 as a whole, which its projection does not see:
        # the scale is observed through e21 alone
        assert np.abs(A12[:, :, 6]).max() < 1e-9 and np.abs(N21[:, :, 6]).max() > 1


def test_huber_by_hand():
    assert R.robustify(3.0, 2.0) == (3.0, 1.0)        # below delta^2 = 4
    assert R.robustify(4.0, 2.0) == (4.0, 1.0)        # at delta^2: still the inlier branch
    assert R.robustify(16.0, 2.0) == (12.0, 0.5)      # 2 * 4 * 2 - 4, 2 / 4


def test_ldlt_solve():
    rng = np.random.default_rng(5)
    M = rng.normal(size=(7, 7))
    H = M @ M.T + 0.1 * np.eye(7)
    b = rng.normal(size=7)
    ok, x = R.ldlt_solve(H, b)
    assert ok and np.allclose(x, np.linalg.solve(H, b), rtol=1e-10, atol=0)
    ok, _ = R.ldlt_solve(-H, b)
    assert not ok


@pytest.mark.parametrize("fix_scale", [False, True])
@pytest.mark.parametrize("cams", [{}, OC.ANISO_PAIR, dict(K1=K_ANISO, K2=C.K_KITTI)])
def test_recovers_the_truth_without_noise(fix_scale, cams):
    p = OC.problem(21, 60, fix_scale=fix_scale, **cams)
    r = R.optimize_sim3(p)
    assert r["second_round"] == 1 and r["n_inliers"] == 60 and r["n_bad"] == 0
    assert r["kept"].all()
    assert OC.pose_error(r, p["truth"]) < TOL
    assert r["stats"][0] <= 5 and r["stats"][1] <= 5
    if fix_scale:
        assert r["s"] == float(p["s12"]) == 1.0  # bit for bit
        assert all(s["H"][6, 6] == 0 and s["b"][6] == 0 for s in r["systems"])


def test_gross_outliers_are_cleared():
    p = OC.problem(22, 100, outlier_frac=0.3, pix_noise=0.5)
    r = R.optimize_sim3(p)
    inl = p["truth"]["inliers"]
    assert r["n_bad"] >= 30 and not r["kept"][~inl].any()
    assert r["second_round"] == 1 and r["stats"][0] <= 5 and 1 <= r["stats"][1] <= 10
    assert r["n_inliers"] == int(r["kept"].sum()) >= 60
    assert np.array_equal(r["kept"], ~((r["chi2"][:, 0] > p["th2"]) | (r["chi2"][:, 1] > p["th2"])))
    assert max(abs(r["s"] - p["truth"]["s"]), np.abs(r["R"] - p["truth"]["R"]).max()) < 1e-2


def test_nine_survivors_return_zero_and_the_input():
    p = OC.problem(23, 12, outlier_frac=0.25)
    r = R.optimize_sim3(p)
    assert r["n_bad"] == 3 and r["second_round"] == 0 and r["n_inliers"] == 0
    assert np.array_equal(r["kept"], p["truth"]["inliers"])  # cleared pairs stay cleared
    assert r["s"] == float(p["s12"])
    assert np.array_equal(r["R"], np.asarray(p["R12"], np.float64))
    assert np.array_equal(r["t"], np.asarray(p["t12"], np.float64))
    assert r["stats"][1] == 0 and r["stats"][3] == 0


def test_no_correspondences():
    p = OC.problem(24, 0)
    r = R.optimize_sim3(p)
    assert r["n_inliers"] == 0 and r["second_round"] == 0 and r["trace"] == []
    assert r["s"] == float(p["s12"])


def test_first_lambda_of_each_round():
    p = OC.problem(25, 80, outlier_frac=0.3, pix_noise=0.5)
    r = R.optimize_sim3(p)
    assert [s["round"] for s in r["systems"]] == [0, 1]
    for s in r["systems"]:
        first = next(t for t in r["trace"] if t["round"] == s["round"])
        assert first["iteration"] == 0
        assert first["lam"] == 1e-5 * np.abs(np.diag(s["H"])).max()
    # the second round's system holds the surviving pairs only
    assert r["systems"][1]["chi2"] < r["systems"][0]["chi2"]


def test_trace_follows_the_policy():
    """Every accepted trial lowers the robust chi2 and shrinks lambda by a factor in [1/3, 2/3];
    rejections multiply it by 2, 4, 8, ...; an iteration holds at most 10 trials."""
    p = OC.problem(26, 300, outlier_frac=0.3, pix_noise=0.5)
    r = R.optimize_sim3(p)
    assert r["stats"][0] <= 5 and r["stats"][1] <= 10
    for rnd in (0, 1):
        tr = [t for t in r["trace"] if t["round"] == rnd]
        ni = 2.0
        for a, b in zip(tr, tr[1:]):
            f = b["lam"] / a["lam"]
            if a["accepted"]:
                assert a["rho"] > 0 and 1 / 3 - 1e-12 <= f <= 2 / 3 + 1e-12
                ni = 2.0
            else:
                assert abs(f - ni) < 1e-9 * ni
                ni *= 2
        for it in range(10):
            assert sum(1 for t in tr if t["iteration"] == it) <= 10
