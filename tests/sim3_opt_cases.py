"""Generators of the OptimizeSim3 test problems (fixed seeds): a known similarity from
sim3_cases.true_sim3 (X1 = s R X2 + t), points 6-30 m ahead of camera 1, pixel noise on both
observations, a share of gross outliers (the pair's point of camera 2 replaced), octaves 0..7,
and a start 2 degrees and 5 % off the truth (the scale exact when it is fixed).  Inputs only."""
import numpy as np

import sim3_cases as C
from camera_cases import K_ANISO

f32 = np.float32
K_KITTI = C.K_KITTI
TH2 = 10.0  # LoopClosing.cc:327


def project(X, K):
    return np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], 1)


def problem(seed, n, outlier_frac=0.0, pix_noise=0.0, fix_scale=False, K1=K_KITTI, K2=K_KITTI,
            th2=TH2):
    """A Context.optimize_sim3 problem dict with its truth (s, R, t, inliers)."""
    rng = np.random.default_rng(seed)
    s, R, t = C.true_sim3(rng, fix_scale)
    X1 = C.points_ahead(rng, n, K1)
    X2 = ((X1 - t) @ R) / s
    obs1 = project(X1, K1) + rng.normal(size=(n, 2)) * pix_noise
    obs2 = project(X2, K2) + rng.normal(size=(n, 2)) * pix_noise
    inl = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.choice(n, n_out, replace=False)
        X2[bad] = C.points_ahead(rng, n_out, K2)
        inl[bad] = False
    _, sigma2 = C.orb_scales()
    inv = (f32(1.0) / sigma2).astype(f32)
    o1 = rng.integers(0, C.NLEVELS, n)
    o2 = np.clip(o1 + rng.integers(-1, 2, n), 0, C.NLEVELS - 1)
    # the start: 2 degrees about a random axis, 5 % in scale, 5 cm in translation
    R0 = C.rot(rng.normal(size=3), np.deg2rad(2.0)) @ R
    s0 = 1.0 if fix_scale else s * 1.05
    t0 = t + rng.uniform(-0.05, 0.05, 3)
    return dict(X1c=X1.astype(f32), X2c=X2.astype(f32), obs1=obs1.astype(f32),
                obs2=obs2.astype(f32), inv_sigma2_1=inv[o1], inv_sigma2_2=inv[o2],
                K1=K1, K2=K2, fix_scale=fix_scale, th2=th2, s12=f32(s0), R12=R0.astype(f32),
                t12=t0.astype(f32), truth=dict(s=s, R=R, t=t, inliers=inl))


def pose_error(r, truth):
    """Largest absolute difference of (s, R, t) from the truth."""
    return max(abs(float(r["s"]) - truth["s"]), float(np.abs(r["R"] - truth["R"]).max()),
               float(np.abs(r["t"] - truth["t"]).max()))


ANISO_PAIR = dict(K1=K_KITTI, K2=K_ANISO)
