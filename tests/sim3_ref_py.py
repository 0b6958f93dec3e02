"""Sequential NumPy restatement of ORB-SLAM2's loop-closure geometry, written from the reference's
text alone (src/Sim3Solver.cc, ORBmatcher::SearchBySim3 in src/ORBmatcher.cc, with the KeyFrame and
MapPoint helpers they call) and independently of the HIP code:

  Sim3Solver   the constructor's products, SetRansacParameters, iterate / find, ComputeSim3
               (Horn 1987), CheckInliers
  search_by_sim3   both projection searches and the agreement pass

float32 arithmetic in the reference's operation order.  Where the reference leaves the result to
OpenCV the choices of DESIGN.md section 2 hold: a cv::Mat product is a dot product summed in double
and rounded to float, then the float add; cv::eigen is a double eigen-solve (np.linalg.eigh) of the
float matrix with the sign fixed; cv::Rodrigues is the closed form in double; Mat::dot and cv::norm
accumulate in double in element order.  The thresholds are the reference's vector<size_t> entries:
9.210 * sigma2 truncated to an integer, compared as a float.

The solver also records, per hypothesis, the two error arrays and the closest approach of any
error to its threshold (min |err / maxErr - 1|), which the GPU tests use to keep clear of ties."""
import math

import numpy as np

f32 = np.float32
f64 = np.float64
INT_MIN = -2 ** 31


def dotd(a, b):
    """A cv::Mat product entry: the dot product summed in double, rounded to float."""
    s = f64(0.0)
    for x, y in zip(a, b):
        s = s + f64(x) * f64(y)
    return f32(s)


def c_int(v):
    """double -> int as x86 converts: NaN and out-of-range values give INT_MIN."""
    if not (v > -2147483649.0 and v < 2147483648.0):
        return INT_MIN
    return int(v)


def camera_to_image(X, K):
    """Sim3Solver::FromCameraToImage over n x 3 float points."""
    fx, fy, cx, cy = [f32(v) for v in K]
    with np.errstate(all="ignore"):
        invz = f32(1.0) / X[:, 2]
        x = X[:, 0] * invz
        y = X[:, 1] * invz
        return np.stack([fx * x + cx, fy * y + cy], 1).astype(f32)


def project(X, sR, t, K):
    """Sim3Solver::Project: Rcw * X + tcw (double-summed rows, float add), then the pinhole."""
    X = X.astype(f32)
    P = np.empty((len(X), 3), f32)
    for r in range(3):
        s = f64(sR[r, 0]) * X[:, 0].astype(f64)
        s = s + f64(sR[r, 1]) * X[:, 1].astype(f64)
        s = s + f64(sR[r, 2]) * X[:, 2].astype(f64)
        P[:, r] = s.astype(f32) + f32(t[r])
    return camera_to_image(P, K)


def max_errors(sigma2):
    """mvnMaxError: 9.210 * sigmaSquare stored in a vector<size_t>, compared as a float."""
    return np.array([f32(int(9.210 * float(f32(s)))) for s in sigma2], f32)


def top_quaternion(N):
    """cv::eigen's first eigenvector as pinned: double eigen-solve of the float matrix, the
    eigenvector of the largest eigenvalue, unit norm, first non-zero of (q0, ...) positive."""
    w, V = np.linalg.eigh(N.astype(f64))
    q = V[:, int(np.argmax(w))].astype(f64)
    q = q / np.sqrt(np.sum(q * q))
    for k in range(4):
        if q[k] != 0:
            if q[k] < 0:
                q = -q
            break
    return q.astype(f32)


def rodrigues(rv):
    """cv::Rodrigues on a double rotation vector: cos I + (1 - cos) k k^T + sin [k]x, to float."""
    theta = np.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2])
    k = rv / theta
    c, s = np.cos(theta), np.sin(theta)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], f64)
    R = np.empty((3, 3), f64)
    for i in range(3):
        for j in range(3):
            R[i, j] = ((c if i == j else f64(0.0)) + ((f64(1.0) - c) * k[i]) * k[j]) + s * Kx[i, j]
    return R.astype(f32)


def compute_sim3(P1, P2, fix_scale):
    """Sim3Solver::ComputeSim3 on two 3 x 3 float matrices whose columns are the three points.
    Returns dict(R, t, s, T12, T21)."""
    P1, P2 = P1.astype(f32), P2.astype(f32)
    with np.errstate(all="ignore"):
        # ComputeCentroid: cv::reduce's float row sums, divided by the column count
        O1 = ((P1[:, 0] + P1[:, 1]) + P1[:, 2]) / f32(3.0)
        O2 = ((P2[:, 0] + P2[:, 1]) + P2[:, 2]) / f32(3.0)
        Pr1 = P1 - O1[:, None]
        Pr2 = P2 - O2[:, None]
        M = np.empty((3, 3), f32)
        for i in range(3):
            for j in range(3):
                M[i, j] = dotd(Pr2[i, :], Pr1[j, :])  # Pr2 * Pr1^T
        N11 = (M[0, 0] + M[1, 1]) + M[2, 2]
        N12 = M[1, 2] - M[2, 1]
        N13 = M[2, 0] - M[0, 2]
        N14 = M[0, 1] - M[1, 0]
        N22 = (M[0, 0] - M[1, 1]) - M[2, 2]
        N23 = M[0, 1] + M[1, 0]
        N24 = M[2, 0] + M[0, 2]
        N33 = (-M[0, 0] + M[1, 1]) - M[2, 2]
        N34 = M[1, 2] + M[2, 1]
        N44 = (-M[0, 0] - M[1, 1]) + M[2, 2]
        N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34],
                      [N14, N24, N34, N44]], f32)
        if np.all(np.isfinite(N)):
            q = top_quaternion(N)
        else:
            q = np.full(4, np.nan, f32)
        vec = q[1:4]
        nrm = np.sqrt((f64(vec[0]) * f64(vec[0]) + f64(vec[1]) * f64(vec[1])) +
                      f64(vec[2]) * f64(vec[2]))  # cv::norm
        ang = f64(math.atan2(float(nrm), float(q[0]))) if np.isfinite(nrm) else f64(np.nan)
        rv = np.array([((f64(2.0) * ang) * f64(vec[k])) / nrm for k in range(3)], f64)
        R = rodrigues(rv)
        P3 = np.empty((3, 3), f32)
        for i in range(3):
            for k in range(3):
                P3[i, k] = dotd(R[i, :], Pr2[:, k])
        if not fix_scale:
            nom, den = f64(0.0), f64(0.0)
            for i in range(3):
                for k in range(3):
                    nom = nom + f64(Pr1[i, k]) * f64(P3[i, k])  # Mat::dot
                    den = den + f64(P3[i, k] * P3[i, k])        # cv::pow(P3, 2), summed in double
            s = f32(nom / den)
        else:
            s = f32(1.0)
        sR = (s * R).astype(f32)
        t = np.array([O1[i] - dotd(sR[i, :], O2) for i in range(3)], f32)
        T12 = np.eye(4, dtype=f32)
        T12[:3, :3] = sR
        T12[:3, 3] = t
        inv = f64(1.0) / f64(s)
        sRinv = (inv * R.T.astype(f64)).astype(f32)
        tinv = np.array([-dotd(sRinv[i, :], t) for i in range(3)], f32)
        T21 = np.eye(4, dtype=f32)
        T21[:3, :3] = sRinv
        T21[:3, 3] = tinv
    return dict(R=R, t=t, s=s, T12=T12, T21=T21)


def ransac_max_iterations(n, probability, min_inliers, max_iterations):
    """Sim3Solver::SetRansacParameters' mRansacMaxIts."""
    def c_log(x):  # libm's log: NaN below zero, -inf at zero
        if x != x or x < 0:
            return float("nan")
        return math.log(x) if x > 0 else float("-inf")

    def c_div(a, b):
        with np.errstate(all="ignore"):
            return float(f64(a) / f64(b))

    with np.errstate(all="ignore"):
        eps = float(f32(min_inliers) / f32(n))
    if min_inliers == n:
        nit = 1
    else:
        e3 = math.pow(eps, 3.0) if math.isfinite(eps) else eps  # pow(float, int): in double
        v = c_div(c_log(1.0 - float(probability)), c_log(1.0 - e3))
        nit = c_int(math.ceil(v) if math.isfinite(v) else v)
    return max(1, min(nit, max_iterations))


class Sim3Solver:
    """The solver after its constructor: X1 / X2 are mvX3Dc1 / mvX3Dc2 (n x 3), sigma2_* the
    level sigmas of the two keys, K1 / K2 = (fx, fy, cx, cy)."""

    def __init__(self, X1, X2, sigma2_1, sigma2_2, K1, K2, fix_scale, probability=0.99,
                 min_inliers=20, max_iterations=300):
        self.X1 = np.ascontiguousarray(X1, f32).reshape(-1, 3)
        self.X2 = np.ascontiguousarray(X2, f32).reshape(-1, 3)
        self.n = len(self.X1)
        self.K1, self.K2 = K1, K2
        self.fix_scale = bool(fix_scale)
        self.max_err1 = max_errors(sigma2_1)
        self.max_err2 = max_errors(sigma2_2)
        self.P1im1 = camera_to_image(self.X1, K1)
        self.P2im2 = camera_to_image(self.X2, K2)
        self.min_inliers = int(min_inliers)
        self.max_its = ransac_max_iterations(self.n, probability, min_inliers, max_iterations)
        self.iterations = 0
        self.best_inliers = 0
        self.best_T12 = np.zeros((4, 4), f32)
        self.best_R = np.zeros((3, 3), f32)
        self.best_t = np.zeros(3, f32)
        self.best_scale = f32(0.0)
        self.best_mask = np.zeros(self.n, bool)
        self.trace = []  # one record per hypothesis run, in order

    def state(self):
        return dict(iterations=self.iterations, best_inliers=self.best_inliers,
                    best_T12=self.best_T12.copy(), best_R=self.best_R.copy(),
                    best_t=self.best_t.copy(), best_scale=self.best_scale,
                    best_mask=self.best_mask.copy())

    def hypothesis(self, draws):
        """One iteration's minimal set (three RandomInt draws through the swap-with-back removal),
        ComputeSim3 and CheckInliers.  Returns dict(idx, sim3, err1, err2, mask, count, margin)."""
        avail = list(range(self.n))
        idx = []
        for j in range(3):
            r = int(draws[j])
            assert 0 <= r < len(avail)
            idx.append(avail[r])
            avail[r] = avail[-1]
            avail.pop()
        P1 = self.X1[idx].T
        P2 = self.X2[idx].T
        h = compute_sim3(P1, P2, self.fix_scale)
        with np.errstate(all="ignore"):
            P2im1 = project(self.X2, h["T12"][:3, :3], h["T12"][:3, 3], self.K1)
            P1im2 = project(self.X1, h["T21"][:3, :3], h["T21"][:3, 3], self.K2)
            d1 = self.P1im1 - P2im1
            d2 = P1im2 - self.P2im2
            e1 = (d1[:, 0].astype(f64) * d1[:, 0].astype(f64) +
                  d1[:, 1].astype(f64) * d1[:, 1].astype(f64)).astype(f32)  # Mat::dot
            e2 = (d2[:, 0].astype(f64) * d2[:, 0].astype(f64) +
                  d2[:, 1].astype(f64) * d2[:, 1].astype(f64)).astype(f32)
            mask = (e1 < self.max_err1) & (e2 < self.max_err2)
            rel = np.concatenate([np.abs(e1.astype(f64) / self.max_err1 - 1.0),
                                  np.abs(e2.astype(f64) / self.max_err2 - 1.0)])
            near = np.minimum(np.abs(e1.astype(f64) / self.max_err1 - 1.0),
                              np.abs(e2.astype(f64) / self.max_err2 - 1.0))
        rel = rel[np.isfinite(rel)]
        return dict(idx=idx, sim3=h, err1=e1, err2=e2, mask=mask, count=int(mask.sum()),
                    margin=float(rel.min()) if len(rel) else float("inf"),
                    near=np.where(np.isfinite(near), near, np.inf))

    def iterate(self, n_iterations, randi):
        """Sim3Solver::iterate(nIterations, bNoMore, vbInliers, nInliers); randi[k] holds the three
        draws of this call's iteration k.  Returns dict(found, T12, mask, n_inliers, no_more, used)
        with mask in correspondence order."""
        out = dict(found=False, T12=np.zeros((4, 4), f32), mask=np.zeros(self.n, bool),
                   n_inliers=0, no_more=False, used=0)
        if self.n < self.min_inliers:
            out["no_more"] = True
            return out
        cur = 0
        while self.iterations < self.max_its and cur < n_iterations:
            h = self.hypothesis(randi[cur])
            cur += 1
            self.iterations += 1
            out["used"] = cur
            self.trace.append(h)
            if h["count"] >= self.best_inliers:
                self.best_mask = h["mask"].copy()
                self.best_inliers = h["count"]
                self.best_T12 = h["sim3"]["T12"].copy()
                self.best_R = h["sim3"]["R"].copy()
                self.best_t = h["sim3"]["t"].copy()
                self.best_scale = h["sim3"]["s"]
                if h["count"] > self.min_inliers:
                    out.update(found=True, T12=self.best_T12.copy(), mask=h["mask"].copy(),
                               n_inliers=h["count"])
                    return out
        if self.iterations >= self.max_its:
            out["no_more"] = True
        return out

    def find(self, randi):
        return self.iterate(self.max_its, randi)


# ------------------------------------------------------------------------------- SearchBySim3
COLS, ROWS = 64, 48  # FRAME_GRID_COLS / ROWS
TH_HIGH = 100


def c_round(v):
    return int(math.floor(abs(float(v)) + 0.5)) * (1 if v >= 0 else -1)


def xform(R, t, x):
    return np.array([dotd(R[r, :], x) + f32(t[r]) for r in range(3)], f32)


class KeyFrameGrid:
    """KeyFrame's mGrid (Frame::AssignFeaturesToGrid / PosInGrid) and GetFeaturesInArea, without
    distortion: image bounds [0, W) x [0, H)."""

    def __init__(self, kps, W, H):
        self.kps = kps
        self.W, self.H = f32(W), f32(H)
        self.invW = f32(COLS) / f32(self.W - f32(0.0))
        self.invH = f32(ROWS) / f32(self.H - f32(0.0))
        self.cells = {}
        for i in range(len(kps)):
            px = c_round(f32(kps["x"][i] - f32(0.0)) * self.invW)
            py = c_round(f32(kps["y"][i] - f32(0.0)) * self.invH)
            if px < 0 or px >= COLS or py < 0 or py >= ROWS:
                continue
            self.cells.setdefault((px, py), []).append(i)

    def in_image(self, u, v):  # KeyFrame::IsInImage
        return bool(u >= 0 and u < self.W and v >= 0 and v < self.H)

    def area(self, x, y, r):
        x0 = max(0, int(math.floor(f32(f32(x - f32(0.0)) - r) * self.invW)))
        if x0 >= COLS:
            return []
        x1 = min(COLS - 1, int(math.ceil(f32(f32(x - f32(0.0)) + r) * self.invW)))
        if x1 < 0:
            return []
        y0 = max(0, int(math.floor(f32(f32(y - f32(0.0)) - r) * self.invH)))
        if y0 >= ROWS:
            return []
        y1 = min(ROWS - 1, int(math.ceil(f32(f32(y - f32(0.0)) + r) * self.invH)))
        if y1 < 0:
            return []
        out = []
        kx, ky = self.kps["x"], self.kps["y"]
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for k in self.cells.get((ix, iy), ()):
                    if abs(f32(kx[k] - x)) < r and abs(f32(ky[k] - y)) < r:
                        out.append(k)
        return out


def predict_scale(max_dist, dist, log_scale, nlevels):
    """MapPoint::PredictScale(currentDist, KeyFrame*): log in double rounded to float, as the
    project's other matchers pin it."""
    ratio = f32(max_dist) / f32(dist)
    ls = f32(math.log(float(ratio))) / log_scale
    n = int(math.ceil(ls))
    if n < 0:
        n = 0
    elif n >= nlevels:
        n = nlevels - 1
    return n


def hamming_rows(a, rows):
    return np.unpackbits(np.bitwise_xor(rows, a[None, :]), axis=1).sum(1)


def _search_one_way(src, dst, G, sR, t, K, th, scale, log_scale, done, reasons):
    """One of SearchBySim3's two loops: the points of `src` searched among the keys of `dst`."""
    fx, fy, cx, cy = [f32(v) for v in K]
    Rs, ts = src["Tcw"][:3, :3].astype(f32), src["Tcw"][:3, 3].astype(f32)
    n = len(src["skip"])
    match = np.full(n, -1, np.int32)
    for i in range(n):
        if src["skip"][i]:
            reasons[i] = "skip"
            continue
        if done[i]:
            reasons[i] = "matched"
            continue
        pc_own = xform(Rs, ts, src["Xw"][i].astype(f32))
        pc = xform(sR, t, pc_own)
        if pc[2] < 0.0:
            reasons[i] = "behind"
            continue
        with np.errstate(all="ignore"):
            invz = f32(f64(1.0) / f64(pc[2]))
            x = pc[0] * invz
            y = pc[1] * invz
            u = fx * x + cx
            v = fy * y + cy
        if not G.in_image(u, v):
            reasons[i] = "outside"
            continue
        max_distance = f32(1.2) * f32(src["max_dist"][i])
        min_distance = f32(0.8) * f32(src["min_dist"][i])
        dist3D = f32(np.sqrt((f64(pc[0]) * f64(pc[0]) + f64(pc[1]) * f64(pc[1])) +
                             f64(pc[2]) * f64(pc[2])))  # cv::norm
        if dist3D < min_distance or dist3D > max_distance:
            reasons[i] = "distance"
            continue
        level = predict_scale(src["max_dist"][i], dist3D, log_scale, len(scale))
        radius = f32(th) * f32(scale[level])
        idx = G.area(u, v, radius)
        if not idx:
            reasons[i] = "empty"
            continue
        best_dist, best = 2 ** 31 - 1, -1
        dists = hamming_rows(src["pdesc"][i], dst["desc"][idx])  # DescriptorDistance, per key
        for k, d in zip(idx, dists):
            o = int(dst["kps"]["octave"][k])
            if o < level - 1 or o > level:
                continue
            if d < best_dist:
                best_dist, best = int(d), k
        if best_dist <= TH_HIGH:
            match[i] = best
            reasons[i] = "candidate"
        else:
            reasons[i] = "octave" if best < 0 else "far"
    return match


def search_by_sim3(kf1, kf2, s12, R12, t12, th, matched12, K, W, H, scale):
    """ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th).  A keyframe is a
    dict(kps, desc, Tcw, Xw, min_dist, max_dist, pdesc, skip) with the point arrays in mvpMapPoints
    order (skip: empty slot or bad point); matched12[i]: -1 none, k >= 0 the point at key k of
    keyframe 2, -2 a point keyframe 2 does not hold.  Returns dict(n_found, match, cand1, cand2,
    reasons1, reasons2)."""
    R12 = np.asarray(R12, f32).reshape(3, 3)
    t12 = np.asarray(t12, f32).reshape(3)
    s12 = f32(s12)
    sR12 = (s12 * R12).astype(f32)
    sR21 = ((f64(1.0) / f64(s12)) * R12.T.astype(f64)).astype(f32)
    t21 = np.array([-dotd(sR21[i, :], t12) for i in range(3)], f32)
    n1, n2 = len(kf1["skip"]), len(kf2["skip"])
    done1, done2 = np.zeros(n1, bool), np.zeros(n2, bool)
    for i in range(n1):
        m = int(matched12[i])
        if m != -1:
            done1[i] = True
            if 0 <= m < n2:
                done2[m] = True
    log_scale = f32(math.log(float(f32(scale[1]))))
    G1 = KeyFrameGrid(kf1["kps"], W, H)
    G2 = KeyFrameGrid(kf2["kps"], W, H)
    r1, r2 = {}, {}
    cand1 = _search_one_way(kf1, kf2, G2, sR21, t21, K, th, scale, log_scale, done1, r1)
    cand2 = _search_one_way(kf2, kf1, G1, sR12, t12, K, th, scale, log_scale, done2, r2)
    match = np.full(n1, -1, np.int32)
    n_found = 0
    for i1 in range(n1):
        i2 = int(cand1[i1])
        if i2 >= 0 and int(cand2[i2]) == i1:
            match[i1] = i2
            n_found += 1
    return dict(n_found=n_found, match=match, cand1=cand1, cand2=cand2, reasons1=r1, reasons2=r2)
