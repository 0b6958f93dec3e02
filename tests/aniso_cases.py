"""Solve cases at the anisotropic camera (camera_cases.K_ANISO), shared by test_oracle_aniso.py
(CPU oracle) and test_gpu_aniso.py (GPU).  Inputs only, plus the measured oracle distances d_o the
issue asks to keep next to each noisy case.

Consistent cases carry no pixel noise and no outliers; their inputs are rounded to float32 as the
API takes them, so the true pose is the minimiser up to that rounding (each test asserts it with
solve_ref_py.gauss_newton_pose before it judges a solver)."""
import numpy as np

from ba_problems import ba_problem
from camera_cases import BF_ANISO, K_ANISO
from synth_problems import flow_problem, p4p_problem, pnp_problem, pose_opt_problem

POSE_TOL = 1e-4   # the project's bar: max abs entry of a 4x4 pose difference
TOL = 1e-4        # the same for BA poses and points
GN_TOL = 1e-5     # where the float64 minimiser must land: a 10x margin under the bar
PNP_PARAMS = (0.99, 10, 300, 4, 0.5, 5.991)
EGO = (0.04, 0.3, 100)   # rp_thres, prior information, iterations of the camera's flow solve
OBJ = (0.01, 0.5, 200)   # ... of an object's

# (seed, n, mono fraction); 1100 and 2049 edges take the four-edges-a-thread and the scratch kernels
POSE_CONSISTENT = [(0, 40, 0.2), (1, 300, 0.0), (2, 300, 1.0), (3, 40, 1.0), (4, 300, 0.2),
                   (5, 1100, 0.2), (6, 2049, 0.2)]
# (seed, n, ego)
FLOW_CONSISTENT = [(0, 64, True), (1, 65, False), (2, 400, True)]
# (seed, n, outlier fraction)
PNP_CASES = [(0, 60, 0.0), (1, 400, 0.0), (2, 60, 0.3), (3, 400, 0.3)]
P4P_CASES = [(0, 15, 0.0), (1, 200, 0.0), (2, 200, 0.3)]
# Local BA graphs.  ba_problem's default perturbation of the initial points (5 cm) is replaced by
# exact initial points: g2o scales its first lambda by the largest diagonal entry, a pose block's,
# which damps the weakly observed depth of distant points so much that the reference's 5 + 10
# iterations leave them centimetres from the truth on consistent data.  With the points exact and
# the poses perturbed (up to 3 cm) the solve has to pull the poses back without disturbing the
# points, and does.
BA_CONSISTENT_KW = dict(pix_noise=0, outlier_frac=0, pt_noise=0, pose_noise=0.003, mono_frac=0,
                        obs_per_pt=(2, 4))
BA_CONSISTENT = [(10, dict(n_kf=4, n_fixed=1, n_pt=100)),
                 (11, dict(n_kf=6, n_fixed=2, n_pt=800)),
                 (12, dict(n_kf=5, n_fixed=1, n_pt=300, kf0_local=False))]

# PoseOptimization with pixel noise and outliers: (seed, n, outlier fraction, mono fraction, d_o).
# d_o is the oracle's own distance to T_min, the float64 least-squares minimiser over the inlier
# set it returns, measured on the CPU (test_oracle_aniso.py re-measures and checks it); the bound
# on a solver's distance to T_min is max(POSE_TOL, 2 d_o).
POSE_NOISY = [(0, 40, 0.1, 0.2, 2.5e-07), (3, 300, 0.2, 0.0, 6.8e-07), (2, 300, 0.3, 1.0, 3.4e-07),
              (9, 300, 0.15, 0.2, 5.6e-07), (6, 40, 0.1, 0.2, 1.7e-05),
              (23, 1100, 0.1, 0.2, 3.0e-07), (24, 2049, 0.1, 0.1, 4.3e-07)]
NEAR_MARGIN = 0.01   # chi2 within 1 % of its threshold: excluded from the flag comparison
NEAR_CAP = 0.02      # at most 2 % of a case's edges may be excluded


def pose_consistent(seed, n, mono):
    return pose_opt_problem(seed, n, outlier_frac=0, pix_noise=0, mono_frac=mono, K=K_ANISO,
                            bf=BF_ANISO)


def pose_noisy(seed, n, out, mono):
    return pose_opt_problem(seed, n, outlier_frac=out, mono_frac=mono, K=K_ANISO, bf=BF_ANISO)


def flow_consistent(seed, n):
    return flow_problem(seed, n, outlier_frac=0, pix_noise=0, K=K_ANISO)


def pnp_case(seed, n, out):
    """Noise-free inliers; the last int(out * n) points (pnp_problem's outlier slots) moved by at
    least 20 px.  Returns (pts3, pts2, T_true, ground-truth inlier indices)."""
    p3, p2, T = pnp_problem(seed, n, outlier_frac=0, pix_noise=0, K=K_ANISO)
    nout = int(out * n)
    if nout:
        rng = np.random.default_rng(1000 + seed)
        ang = rng.uniform(0, 2 * np.pi, nout)
        r = rng.uniform(20, 60, nout)
        p2[-nout:] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1).astype(np.float32)
    return p3, p2, T, np.arange(n - nout)


def p4p_case(seed, n, out):
    """As pnp_case for the relocalisation PnPsolver: (pts3, pts2, sigma2, T_true, inlier mask)."""
    p3, p2, s2, T = p4p_problem(seed, n, outlier_frac=0, pix_noise=0, K=K_ANISO)
    nout = int(out * n)
    mask = np.ones(n, bool)
    if nout:
        rng = np.random.default_rng(2000 + seed)
        idx = rng.choice(n, nout, replace=False)
        ang = rng.uniform(0, 2 * np.pi, nout)
        # chi2 = d^2 / sigma2 against 5.991 with sigma2 up to 1.2^14: 20 px would pass at the
        # coarsest octaves, so the displacement scales with the octave's sigma
        r = rng.uniform(20, 60, nout) * np.sqrt(s2[idx])
        p2[idx] += np.stack([r * np.cos(ang), r * np.sin(ang)], 1).astype(np.float32)
        mask[idx] = False
    return p3, p2, s2, T, mask


def ba_consistent(seed, kw):
    return ba_problem(seed, K=K_ANISO, bf=BF_ANISO, **BA_CONSISTENT_KW, **kw)
