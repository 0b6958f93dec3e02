"""Float64 NumPy edge models of the solves (SURVEY rows D1, D2/D3, D5/D6 and the local BA), written
from the reference's edge definitions (Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h,cpp} and
the information matrices Optimizer.cc sets), not from oracle/ or csrc/.

These are not solvers of the reference's kind: nothing here restates g2o's Levenberg-Marquardt
policy (lambda, rho, stop rules, re-classification rounds).  They evaluate each edge's error at a
given pose, which is a fact about any correct solver's output whatever its trajectory, and
gauss_newton_pose finds the float64 minimiser of a residual function by the plainest means
(numeric Jacobian, damped normal equations).

Conventions: T is a 4x4 world-to-camera matrix (Tcw); K = (fx, fy, cx, cy); everything is
promoted to float64 on entry.  Pinned in tests/test_solve_ref_py.py."""
import numpy as np

CHI2_MONO = 5.991    # Optimizer.cc:3257 chi2Mono
CHI2_STEREO = 7.815  # Optimizer.cc:3258 chi2Stereo
FLOW_INFO = 0.1      # Optimizer.cc:466 info_flow (EdgeSE3ProjectFlow2)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def transform(T, X):
    """SE3Quat::map: R X + t for the rows of X."""
    T, X = _f64(T), _f64(X)
    return X @ T[:3, :3].T + T[:3, 3]


def cam_project(pc, K):
    """Edge*::cam_project (types_six_dof_expmap.cpp): [fx x/z + cx, fy y/z + cy]."""
    fx, fy, cx, cy = (float(k) for k in K)
    pc = _f64(pc)
    iz = 1.0 / pc[..., 2]
    return np.stack([pc[..., 0] * iz * fx + cx, pc[..., 1] * iz * fy + cy], -1)


def cam_project_stereo(pc, K, bf):
    """EdgeStereoSE3ProjectXYZ*::cam_project: [u, v, u - bf / z]."""
    uv = cam_project(pc, K)
    return np.concatenate([uv, uv[..., :1] - float(bf) / _f64(pc)[..., 2:3]], -1)


def pose_edge_errors(T, Xw, obs, K, bf):
    """Per-edge error of EdgeSE3ProjectXYZOnlyPose (obs[:, 2] = uR < 0: monocular, the third
    component is 0) or EdgeStereoSE3ProjectXYZOnlyPose (uR >= 0): obs - cam_project(T Xw)
    (types_six_dof_expmap.h:154-158, 185-189).  Returns (errors (n, 3), mono mask)."""
    obs = _f64(obs)
    mono = obs[:, 2] < 0
    e = obs - cam_project_stereo(transform(T, Xw), K, bf)
    e[mono, 2] = 0.0
    return e, mono


def chi2_pose_edges(T, Xw, obs, inv_sigma2, K, bf):
    """Per-edge chi2 = e^T (I * invSigma2) e of Optimizer::PoseOptimization's edges
    (information: Optimizer.cc:3187-3188 monocular, 3223-3225 stereo)."""
    e, _ = pose_edge_errors(T, Xw, obs, K, bf)
    return (e * e).sum(1) * _f64(inv_sigma2)


def pose_outlier_flags(T, Xw, obs, inv_sigma2, K, bf, margin=0.0):
    """mvbOutlier as the last classification of PoseOptimization sets it (Optimizer.cc:3283,
    3312): chi2 > 5.991 (mono) / 7.815 (stereo).  Also returns the mask of edges whose chi2 lies
    within the relative `margin` of its threshold (to be excluded from exact comparisons)."""
    chi2 = chi2_pose_edges(T, Xw, obs, inv_sigma2, K, bf)
    th = np.where(_f64(obs)[:, 2] < 0, CHI2_MONO, CHI2_STEREO)
    return chi2 > th, np.abs(chi2 - th) <= margin * th


def flow_points_world(obs, depth, Tcw_last, K):
    """The 3-D point of an EdgeSE3ProjectFlow2: the last frame's pixel back-projected at its depth
    and moved to the world by Twl (types_six_dof_expmap.h:445-446)."""
    fx, fy, cx, cy = (float(k) for k in K)
    obs, depth = _f64(obs), _f64(depth)
    pl = np.stack([(obs[:, 0] - cx) * depth / fx, (obs[:, 1] - cy) * depth / fy, depth], 1)
    return transform(np.linalg.inv(_f64(Tcw_last)), pl)


def flow_residuals(T, flow_vertices, obs, flow_meas, depth, Tcw_last, K):
    """Errors of the flow solve's two edge kinds at pose T and flow-vertex estimates
    flow_vertices (n, 2):
      EdgeSE3ProjectFlow2  (obs + est) - cam_project(T Twl Xl)   (types_six_dof_expmap.h:439-448)
      EdgeFlowPrior        est - measured flow                    (types_six_dof_expmap.h:416-421)
    Returns (e_proj (n, 2), e_prior (n, 2))."""
    Xw = flow_points_world(obs, depth, Tcw_last, K)
    est = _f64(flow_vertices)
    e_proj = (_f64(obs) + est) - cam_project(transform(T, Xw), K)
    return e_proj, est - _f64(flow_meas)


def flow_chi2(T, flow_vertices, obs, flow_meas, depth, Tcw_last, K, prior_info):
    """chi2 of both edge kinds: information 0.1 I on the projection edge (Optimizer.cc:466) and
    prior_info I on the prior (0.3 for the camera, Optimizer.cc:501; 0.5 for an object, :2277)."""
    ep, eq = flow_residuals(T, flow_vertices, obs, flow_meas, depth, Tcw_last, K)
    return FLOW_INFO * (ep * ep).sum(1), float(prior_info) * (eq * eq).sum(1)


def ba_residuals(T_kf, X, edges, K, bf):
    """Errors of the local BA's edges: EdgeSE3ProjectXYZ (uR < 0; third component 0) and
    EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.h:91-96, 123-128): obs - cam_project(T_kf X_pt).
    edges: dict(pt, kf, obs (n, 3)).  Returns (errors (n, 3), mono mask)."""
    T_kf, X = _f64(T_kf), _f64(X)
    pt, kf = np.asarray(edges["pt"]), np.asarray(edges["kf"])
    obs = _f64(edges["obs"]).reshape(-1, 3)
    R, t = T_kf[kf, :3, :3], T_kf[kf, :3, 3]
    pc = np.einsum("nij,nj->ni", R, X[pt]) + t
    mono = obs[:, 2] < 0
    e = obs - cam_project_stereo(pc, K, bf)
    e[mono, 2] = 0.0
    return e, mono


def reprojection_sq_error(T, pts3, pts2, K):
    """Per-point squared pixel distance between pts2 and the projection of pts3 at T."""
    d = _f64(pts2) - cam_project(transform(T, pts3), K)
    return (d * d).sum(1)


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    """exp of a twist (omega, upsilon) as a 4x4 matrix (closed form)."""
    xi = _f64(xi)
    w, v = xi[:3], xi[3:]
    th = np.linalg.norm(w)
    W = hat(w)
    if th < 1e-10:
        R = np.eye(3) + W + 0.5 * W @ W
        V = np.eye(3) + 0.5 * W + W @ W / 6.0
    else:
        a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
        R = np.eye(3) + a * W + b * W @ W
        V = np.eye(3) + b * W + c * W @ W
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = V @ v
    return T


def gauss_newton_pose(residual_fn, T0, iters=100, h=1e-6, step_tol=1e-13):
    """The float64 minimiser of sum(residual_fn(T)^2) over SE(3), from T0: T <- exp(d) T with d
    from damped normal equations on a central-difference Jacobian; the damping grows on a
    rejected step and shrinks on an accepted one.  A plain least-squares tool to locate a
    minimum, not the reference's optimiser."""
    T = _f64(T0).copy()
    r = np.ravel(residual_fn(T))
    cost = float(r @ r)
    mu = 1e-6
    for _ in range(iters):
        J = np.empty((r.size, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            J[:, k] = (np.ravel(residual_fn(se3_exp(d) @ T)) -
                       np.ravel(residual_fn(se3_exp(-d) @ T))) / (2 * h)
        A, g = J.T @ J, J.T @ r
        moved = done = False
        while mu < 1e12:
            d = np.linalg.solve(A + mu * np.diag(np.diag(A) + 1e-12), -g)
            Tn = se3_exp(d) @ T
            rn = np.ravel(residual_fn(Tn))
            cn = float(rn @ rn)
            if np.isfinite(cn) and cn <= cost:
                T, r, moved = Tn, rn, True
                done = np.abs(d).max() < step_tol or cost - cn <= 1e-30 + 1e-16 * cost
                cost = cn
                mu = max(mu * 0.1, 1e-12)
                break
            mu *= 10.0
        if not moved or done:
            break
    return T


def pose_residual_fn(Xw, obs, inv_sigma2, K, bf, keep=None):
    """sqrt(information)-weighted residual vector of the pose edges selected by `keep`."""
    Xw, obs, s = _f64(Xw), _f64(obs), np.sqrt(_f64(inv_sigma2))
    if keep is not None:
        Xw, obs, s = Xw[keep], obs[keep], s[keep]

    def fn(T):
        e, _ = pose_edge_errors(T, Xw, obs, K, bf)
        return e * s[:, None]
    return fn


def flow_residual_fn(obs, flow_meas, depth, Tcw_last, K):
    """Residual of the flow solve as a function of the pose alone, the flow vertices held at their
    measurements.  Eliminating a flow vertex from 0.1 |obs + est - p|^2 + c |est - flow|^2 leaves
    (0.1 c / (0.1 + c)) |p - obs - flow|^2, so the pose minimiser is that of this residual."""
    def fn(T):
        return flow_residuals(T, flow_meas, obs, flow_meas, depth, Tcw_last, K)[0]
    return fn


def reprojection_residual_fn(pts3, pts2, K, keep=None):
    pts3, pts2 = _f64(pts3), _f64(pts2)
    if keep is not None:
        pts3, pts2 = pts3[keep], pts2[keep]

    def fn(T):
        return _f64(pts2) - cam_project(transform(T, pts3), K)
    return fn
