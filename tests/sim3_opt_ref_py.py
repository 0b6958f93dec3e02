"""Sequential float64 NumPy restatement of Optimizer::OptimizeSim3 (reference src/Optimizer.cc:
3934-4129), written from the reference's text alone and independently of the HIP code:

  Sim3               g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h): the four-branch exponential, the
                     product, the inverse and map, on an unnormalised Eigen quaternion
  edge_errors        EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ::computeError
                     (types/types_seven_dof_expmap.h)
  numeric_jacobians  BaseBinaryEdge::linearizeOplus (core/base_binary_edge.hpp:131-205): the
                     central difference at 1e-9 through VertexSim3Expmap::oplusImpl
  robustify          RobustKernelHuber (core/robust_kernel_impl.cpp)
  ldlt_solve         LinearSolverDense: Eigen's LDLT with diagonal pivoting, isPositive()
  lm_round           OptimizationAlgorithmLevenberg::solve inside SparseOptimizer::optimize, with
                     ORB-SLAM2's two added stops
  optimize_sim3      both rounds, the removal of the bad pairs, the inlier counts

Pins: the inputs are float and promoted to double; deltaHuber is sqrtf(th2) promoted; chi2() is the
plain e . (Omega e); an edge keeps the error of the last computeActiveErrors, which is the last
trial's state (after a rejected trial the vertex is popped, the edges' errors are not), so the
inlier tests read the last trial's errors; a failed first solve of a round applies a zero increment
(the reference's is uninitialised).  Edge sums are np.sum over the pairs; the order is rounding.

Every trial is traced (round, iteration, lambda, chi2, rho, accepted), and so are each round's
first system and the closest approach of any tested chi2 to th2 (min |chi2 / th2 - 1|), which the GPU
tests use to keep clear of ties."""
import math

import numpy as np

f32 = np.float32
f64 = np.float64
EPS = 1e-5
DELTA = 1e-9
DBL_MAX = float(np.finfo(f64).max)


# ------------------------------------------------------------------- Eigen quaternions (x, y, z, w)
def quat_from_R(R):
    """Eigen::Quaterniond(Matrix3d): the trace branch, else the largest diagonal entry's."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4, f64)
    if t > 0:
        s = math.sqrt(t + 1.0)
        q[3] = 0.5 * s
        s = 0.5 / s
        q[0] = (R[2, 1] - R[1, 2]) * s
        q[1] = (R[0, 2] - R[2, 0]) * s
        q[2] = (R[1, 0] - R[0, 1]) * s
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        s = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (R[k, j] - R[j, k]) * s
        q[j] = (R[j, i] + R[i, j]) * s
        q[k] = (R[k, i] + R[i, k]) * s
    return q


def quat_to_R(q):
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]], f64)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], f64)


def quat_rotate(q, v):
    """q * v (Eigen's _transformVector) over (..., 3) vectors."""
    qv = q[:3]
    uv = np.cross(qv, v)
    uv = uv + uv
    return v + q[3] * uv + np.cross(qv, uv)


def skew(o):
    return np.array([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]], f64)


class Sim3:
    def __init__(self, q, t, s):
        self.q, self.t, self.s = np.asarray(q, f64), np.asarray(t, f64), float(s)

    @staticmethod
    def from_R(R, t, s):
        return Sim3(quat_from_R(np.asarray(R, f64)), t, s)

    @staticmethod
    def exp(update):
        """Sim3(const Vector7d&), sim3.h:70-142; also returns the branch taken (0..3)."""
        update = np.asarray(update, f64)
        omega, upsilon, sigma = update[:3], update[3:6], float(update[6])
        theta = math.sqrt(float(np.sum(omega * omega)))
        Om = skew(omega)
        s = math.exp(sigma)
        Om2 = Om @ Om
        I = np.eye(3)
        if abs(sigma) < EPS:
            C = 1.0
            if theta < EPS:
                A, B = 1.0 / 2.0, 1.0 / 6.0
                R = I + Om + Om @ Om
                branch = 0
            else:
                theta2 = theta * theta
                A = (1 - math.cos(theta)) / theta2
                B = (theta - math.sin(theta)) / (theta2 * theta)
                R = I + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / (theta * theta) * Om2
                branch = 1
        else:
            C = (s - 1) / sigma
            if theta < EPS:
                sigma2 = sigma * sigma
                A = ((sigma - 1) * s + 1) / sigma2
                B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
                R = I + Om + Om2
                branch = 2
            else:
                R = I + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / (theta * theta) * Om2
                a = s * math.sin(theta)
                b = s * math.cos(theta)
                theta2 = theta * theta
                sigma2 = sigma * sigma
                c = theta2 + sigma2
                A = (a * sigma + (1 - b) * theta) / (theta * c)
                B = (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2
                branch = 3
        W = A * Om + B * Om2 + C * I
        S = Sim3(quat_from_R(R), W @ upsilon, s)
        S.branch = branch
        return S

    def R(self):
        return quat_to_R(self.q)

    def map(self, X):
        return self.s * quat_rotate(self.q, np.asarray(X, f64)) + self.t

    def inverse(self):
        qc = np.array([-self.q[0], -self.q[1], -self.q[2], self.q[3]], f64)
        return Sim3(qc, quat_rotate(qc, (-1.0 / self.s) * self.t), 1.0 / self.s)

    def __mul__(self, o):
        return Sim3(quat_mul(self.q, o.q), self.s * quat_rotate(self.q, o.t) + self.t,
                    self.s * o.s)


def oplus(S, update, fix_scale):
    """VertexSim3Expmap::oplusImpl."""
    u = np.array(update, f64)
    if fix_scale:
        u[6] = 0
    return Sim3.exp(u) * S


# ------------------------------------------------------------------------------------- the edges
def _pinhole(P, K):
    with np.errstate(all="ignore"):
        return np.stack([P[:, 0] / P[:, 2] * K[0] + K[2], P[:, 1] / P[:, 2] * K[1] + K[3]], 1)


def edge_errors(S, pr):
    """(e12, e21), n x 2 each: obs1 - cam_map1(project(S.map(X2c))) and
    obs2 - cam_map2(project(S.inverse().map(X1c)))."""
    e12 = pr["obs1"] - _pinhole(S.map(pr["X2c"]), pr["K1"])
    e21 = pr["obs2"] - _pinhole(S.inverse().map(pr["X1c"]), pr["K2"])
    return e12, e21


def chi2_of(e, w):
    """BaseEdge::chi2 with the information w I: e . (Omega e)."""
    return e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])


def numeric_jacobians(S, pr, fix_scale):
    """(J12, J21), n x 2 x 7: column d = (1 / 2e-9) (e(+1e-9 e_d) - e(-1e-9 e_d))."""
    n = len(pr["X1c"])
    J12, J21 = np.zeros((n, 2, 7), f64), np.zeros((n, 2, 7), f64)
    scalar = 1.0 / (2 * DELTA)
    for d in range(7):
        add = np.zeros(7, f64)
        add[d] = DELTA
        p12, p21 = edge_errors(oplus(S, add, fix_scale), pr)
        add[d] = -DELTA
        m12, m21 = edge_errors(oplus(S, add, fix_scale), pr)
        J12[:, :, d] = scalar * (p12 - m12)
        J21[:, :, d] = scalar * (p21 - m21)
    return J12, J21


def robustify(e, delta):
    """RobustKernelHuber::robustify with dsqr = delta * delta: (rho, rho')."""
    dsqr = delta * delta
    if e <= dsqr:
        return e, 1.0
    sqrte = math.sqrt(e)
    return 2 * sqrte * delta - dsqr, delta / sqrte


def _robust(c, delta):
    with np.errstate(all="ignore"):
        dsqr = delta * delta
        sq = np.sqrt(c)
        inl = c <= dsqr
        return np.where(inl, c, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)


def ldlt_solve(H, b):
    """Eigen::LDLT<MatrixXd>::compute + isPositive + solve: (ok, x).  Left-looking, the pivot is the
    largest remaining diagonal entry; not positive when a pivot is negative."""
    n = len(b)
    A = np.array(H, f64)
    perm = list(range(n))
    L = np.zeros((n, n), f64)
    D = np.zeros(n, f64)
    positive = True
    with np.errstate(all="ignore"):
        for k in range(n):
            p, best = k, abs(A[k, k])
            for i in range(k + 1, n):
                if abs(A[i, i]) > best:
                    p, best = i, abs(A[i, i])
            if p != k:
                A[[k, p], :] = A[[p, k], :]
                A[:, [k, p]] = A[:, [p, k]]
                L[[k, p], :k] = L[[p, k], :k]
                perm[k], perm[p] = perm[p], perm[k]
            d = A[k, k]
            for c in range(k):
                d -= L[k, c] * L[k, c] * D[c]
            D[k] = d
            if d < 0:
                positive = False
            for i in range(k + 1, n):
                s = A[i, k]
                for c in range(k):
                    s -= L[i, c] * L[k, c] * D[c]
                L[i, k] = s / d if d != 0 else 0.0
            L[k, k] = 1.0
        if not positive:
            return False, None
        y = np.array([b[perm[i]] for i in range(n)], f64)
        for i in range(n):
            for c in range(i):
                y[i] -= L[i, c] * y[c]
        for i in range(n):
            y[i] = y[i] / D[i] if D[i] != 0 else 0.0
        for i in range(n - 1, -1, -1):
            for r in range(i + 1, n):
                y[i] -= L[r, i] * y[r]
        x = np.zeros(n, f64)
        for i in range(n):
            x[perm[i]] = y[i]
    return True, x


# ------------------------------------------------------------------------------- the optimisation
class _Graph:
    """The active edges (pairs with act set) and their last computed errors."""

    def __init__(self, pr, fix_scale, delta):
        self.pr, self.fix_scale, self.delta = pr, fix_scale, delta
        n = len(pr["X1c"])
        self.act = np.ones(n, bool)
        self.c12 = np.zeros(n, f64)
        self.c21 = np.zeros(n, f64)

    def sub(self):
        a = self.act
        p = self.pr
        return dict(X1c=p["X1c"][a], X2c=p["X2c"][a], obs1=p["obs1"][a], obs2=p["obs2"][a],
                    K1=p["K1"], K2=p["K2"]), p["w1"][a], p["w2"][a]

    def compute_active_errors(self, S):
        """computeActiveErrors + activeRobustChi2."""
        p, w1, w2 = self.sub()
        e12, e21 = edge_errors(S, p)
        self.e12, self.e21 = e12, e21
        self.last_state = S
        self.c12[self.act] = chi2_of(e12, w1)
        self.c21[self.act] = chi2_of(e21, w2)
        r12, _ = _robust(self.c12[self.act], self.delta)
        r21, _ = _robust(self.c21[self.act], self.delta)
        return float(np.sum(r12 + r21))

    def build_system(self, S):
        """linearizeOplus + constructQuadraticForm of every active edge at S (whose errors
        compute_active_errors has just left in e12 / e21): (H, b)."""
        p, w1, w2 = self.sub()
        J12, J21 = numeric_jacobians(S, p, self.fix_scale)
        H = np.zeros((7, 7), f64)
        b = np.zeros(7, f64)
        with np.errstate(all="ignore"):
            for J, e, w, c in ((J12, self.e12, w1, self.c12[self.act]),
                               (J21, self.e21, w2, self.c21[self.act])):
                _, r1 = _robust(c, self.delta)
                omega_r = -(w[:, None] * e) * r1[:, None]
                wo = r1 * w
                b += np.sum(np.einsum("nra,nr->na", J, omega_r), 0)
                H += np.sum(np.einsum("nra,n,nrb->nab", J, wo, J), 0)
        return H, b


def lm_round(G, S, iterations, rnd, trace, systems):
    """SparseOptimizer::optimize(iterations) after initializeOptimization(): returns the estimate
    and (iterations run, trials run)."""
    lam = ni = 0.0
    n_bad = 0
    chi2_check = 0.0
    x = np.zeros(7, f64)
    its = trials = 0
    for it in range(iterations):
        # ---- OptimizationAlgorithmLevenberg::solve(it)
        current = G.compute_active_errors(S)
        temp = current
        ini = current
        H, b = G.build_system(S)
        if it == 0:
            lam = 1e-5 * max(abs(H[j, j]) for j in range(7))
            ni = 2.0
            n_bad = 0
            systems.append(dict(round=rnd, H=H.copy(), b=b.copy(), chi2=current, lam=lam))
        rho = 0.0
        qmax = 0
        while True:
            backup = S
            ok2, sol = ldlt_solve(H + lam * np.eye(7), b)
            if ok2:
                x = sol
            if G.fix_scale:
                x[6] = 0  # oplusImpl writes through the solver's increment
            with np.errstate(all="ignore"):
                S = oplus(backup, x, G.fix_scale)
                temp = G.compute_active_errors(S)
                last_chi = temp
                if not ok2:
                    temp = DBL_MAX
                scale = float(np.sum(x * (lam * x + b))) + 1e-3
                rho = (current - temp) / scale
            lam_used = lam
            accepted = bool(rho > 0 and math.isfinite(temp))
            if accepted:
                alpha = 1.0 - (2 * rho - 1) ** 3
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current = temp
            else:
                lam *= ni
                ni *= 2
                S = backup
            qmax += 1
            trials += 1
            trace.append(dict(round=rnd, iteration=it, lam=lam_used, chi2=last_chi, rho=rho,
                              accepted=accepted))
            if not (rho < 0 and qmax < 10):
                break
        its += 1
        ok = True
        if qmax == 10 or rho == 0:
            ok = False
        else:
            if (ini - current) * 1e3 < ini:
                n_bad += 1
            else:
                n_bad = 0
            if n_bad >= 3:
                ok = False
        # ---- SparseOptimizer::optimize's added stop, on the edges' last computed errors
        if chi2_check < last_chi and it > 0:
            ok = False
        chi2_check = last_chi
        if not ok:
            break
    return S, its, trials


def problem_arrays(p):
    """A Context.optimize_sim3 problem dict as float64 arrays (float inputs promoted)."""
    a = lambda k, c: np.asarray(p[k], f32).reshape(-1, c).astype(f64)
    return dict(X1c=a("X1c", 3), X2c=a("X2c", 3), obs1=a("obs1", 2), obs2=a("obs2", 2),
                w1=np.asarray(p["inv_sigma2_1"], f32).astype(f64).reshape(-1),
                w2=np.asarray(p["inv_sigma2_2"], f32).astype(f64).reshape(-1),
                K1=[float(f32(v)) for v in p["K1"]], K2=[float(f32(v)) for v in p["K2"]])


def optimize_sim3(p):
    """Optimizer::OptimizeSim3 on a problem dict(X1c, X2c, obs1, obs2, inv_sigma2_1, inv_sigma2_2,
    K1, K2, fix_scale, th2, s12, R12, t12).  Returns dict(n_inliers, n_bad, second_round, s, R, t,
    kept, chi2 (n x 2, of every pair at the last tested state), stats, trace, systems, margin)."""
    pr = problem_arrays(p)
    n = len(pr["X1c"])
    th2 = float(f32(p["th2"]))
    delta = float(f32(math.sqrt(f32(p["th2"]))))  # const float deltaHuber = sqrt(th2)
    fix = bool(p["fix_scale"])
    s0 = float(f32(p["s12"]))
    R0 = np.asarray(p["R12"], f32).reshape(3, 3).astype(f64)
    t0 = np.asarray(p["t12"], f32).reshape(3).astype(f64)
    out = dict(n_inliers=0, n_bad=0, second_round=0, s=s0, R=R0, t=t0, kept=np.zeros(n, bool),
               chi2=np.zeros((n, 2), f64), stats=[0, 0, 0, 0], trace=[], systems=[],
               margin=np.inf)
    if n == 0:
        return out
    S = Sim3.from_R(R0, t0, s0)
    G = _Graph(pr, fix, delta)

    def margin(c12, c21):
        with np.errstate(all="ignore"):
            m = np.abs(np.concatenate([c12, c21]) / th2 - 1.0)
        return float(np.min(m[np.isfinite(m)])) if np.any(np.isfinite(m)) else np.inf

    S, out["stats"][0], out["stats"][2] = lm_round(G, S, 5, 0, out["trace"], out["systems"])
    bad = (G.c12 > th2) | (G.c21 > th2)
    out["margin"] = margin(G.c12, G.c21)
    out["chi2"] = np.stack([G.c12, G.c21], 1).copy()
    out["n_bad"] = int(bad.sum())
    out["kept"] = ~bad
    G.act = ~bad
    if n - out["n_bad"] < 10:
        return out
    S, out["stats"][1], out["stats"][3] = lm_round(G, S, 10 if out["n_bad"] > 0 else 5, 1,
                                                   out["trace"], out["systems"])
    # the removed pairs' chi2 is evaluated at the same state as the survivors' (the reference no
    # longer holds their edges; the kernel reports it, and the tests keep it clear of th2 too)
    c12, c21 = G.c12.copy(), G.c21.copy()
    if bad.any():
        q = {k: (v[bad] if isinstance(v, np.ndarray) else v) for k, v in pr.items()}
        e12, e21 = edge_errors(G.last_state, q)
        c12[bad] = chi2_of(e12, pr["w1"][bad])
        c21[bad] = chi2_of(e21, pr["w2"][bad])
    out["margin"] = min(out["margin"], margin(c12, c21))
    out["chi2"] = np.stack([c12, c21], 1)
    out["kept"] = ~bad & ~((c12 > th2) | (c21 > th2))
    out["n_inliers"] = int(out["kept"].sum())
    out["second_round"] = 1
    out["s"], out["R"], out["t"] = S.s, S.R(), S.t.copy()
    return out
