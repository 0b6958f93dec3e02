"""Inputs of the two matchers of the vocabulary path: Relocalization's SearchByProjection(Frame&,
KeyFrame*, sAlreadyFound, th, ORBdist) (ORBmatcher.cc:2104-2231) and LocalMapping's
SearchForTriangulation (ORBmatcher.cc:1032-1131).

Inputs only: expected outputs come from the CPU oracle at test time, and the properties a case
exists for are asserted from the oracle's result or from the Python restatement in
test_oracle_reloc_match.py.  Every case carries `tags`: the indices its property speaks about.

The kitti cases use the reference's kitti_sample frames (match_problems) and FeatureVectors from
the test vocabulary; the hand-built cases place every key, point and vocabulary node by hand
(bow_problems.feature_vector), a few hundred keys at most."""
import os

import numpy as np

import bow_problems as BP
import match_problems as MP

K, BF, W, H = MP.K, MP.BF, MP.W, MP.H
KP = BP.KP_DTYPE
VOC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "test_voc_k10l6.txt")
f32 = np.float32
CELL_W, CELL_H = W / 64.0, H / 48.0  # Frame's grid elements (FRAME_GRID_COLS x FRAME_GRID_ROWS)
_CACHE = {}


# ------------------------------------------------------------------ small helpers
def flipped(rng, d, k):
    """d with exactly k bits flipped: Hamming distance k."""
    d = d.copy()
    for b in rng.choice(256, int(k), replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def rot_y(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def pose(R, C):
    """Tcw (float32) of a camera with rotation Rcw and centre C."""
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = -R @ np.asarray(C, np.float64)
    return T.astype(f32)


def world_point(T, u, v, z):
    """The world point that projects to (u, v) at camera depth z under Tcw = T (float32)."""
    xc = np.array([(u - K[2]) * z / K[0], (v - K[3]) * z / K[1], z], np.float64)
    Ti = np.linalg.inv(T.astype(np.float64))
    return (Ti[:3, :3] @ xc + Ti[:3, 3]).astype(f32)


def dist3d(T, X):
    """|X - Ow| as the matcher computes it: Ow = -Rcw^T tcw and the norm accumulated in double,
    each rounded to float once."""
    T = T.astype(f32)
    Ow = np.zeros(3, f32)
    for r in range(3):
        s = 0.0
        for k in range(3):
            s += float(T[k, r]) * float(T[k, 3])
        Ow[r] = -f32(s)
    s = 0.0
    for k in range(3):
        d = f32(f32(X[k]) - Ow[k])
        s += float(d) * float(d)
    return f32(np.sqrt(s))


def level_dists(d, level):
    """(min_dist, max_dist) that put PredictScale at `level` for camera distance d, mid-level: the
    ratio max_dist / d is 1.2^(level - 0.5), away from the ceil's edges."""
    dmax = f32(float(d) * 1.2 ** (level - 0.5))
    return f32(dmax / f32(1.2 ** 7)), dmax


def sites(n, x0=60.0, y0=45.0, dx=70.0, dy=58.0, cols=16):
    """n image positions far enough apart that no search window holds another site's key."""
    out = [(x0 + dx * (i % cols), y0 + dy * (i // cols)) for i in range(n)]
    assert all(y < H - 30 for _, y in out)
    return out


def compute_f12(T1, T2):
    """LocalMapping::ComputeF12 = K^-T [t12]x R12 K^-1 as the oracle and the product pin it: double
    from the float poses and intrinsics in this operation order, one rounding to float."""
    T1 = T1.astype(f32).astype(np.float64)
    T2 = T2.astype(f32).astype(np.float64)
    R12 = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            s = 0.0
            for k in range(3):
                s += T1[r, k] * T2[c, k]
            R12[r, c] = s
    t12 = np.zeros(3)
    for r in range(3):
        s = 0.0
        for c in range(3):
            s += R12[r, c] * T2[c, 3]
        t12[r] = -s + T1[r, 3]
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    fx, fy, cx, cy = [float(f32(v)) for v in K]
    Ki = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]])

    def mul(A, B, At=False):
        out = np.zeros((3, 3))
        for r in range(3):
            for c in range(3):
                s = 0.0
                for k in range(3):
                    s += (A[k, r] if At else A[r, k]) * B[k, c]
                out[r, c] = s
        return out
    return mul(mul(mul(Ki, tx, At=True), R12), Ki).astype(f32)


# ------------------------------------------------------------------ SearchByProjection(F, KF)
T_HAND = pose(rot_y(0.02), (0.1, -0.05, 0.3))
T_AXIS = np.eye(4, dtype=f32)   # Rcw = I: camera coordinates are Xw + tcw, exactly
T_AXIS[:3, 3] = (0.1, -0.05, 0.3)


class _Sbp:
    """Builder of one hand-built SearchByProjection(F, KF) problem."""

    def __init__(self, T, th, orb_dist, seed):
        self.T, self.th, self.orb = T, float(th), int(orb_dist)
        self.rng = np.random.default_rng(seed)
        self.keys, self.kdesc, self.kbound = [], [], []
        self.pts = []
        self.tags = {}

    def tag(self, name, idx):
        self.tags.setdefault(name, []).append(int(idx))

    def key(self, x, y, octave, desc, angle=0.0, bound=0):
        assert 0 <= x < W and 0 <= y < H
        k = np.zeros(1, KP)
        k["x"], k["y"], k["octave"], k["angle"], k["size"] = x, y, octave, angle, 31
        self.keys.append(k)
        self.kdesc.append(np.asarray(desc, np.uint8))
        self.kbound.append(bound)
        return len(self.keys) - 1

    def point(self, X, dmin, dmax, desc, angle=0.0, skip=0):
        self.pts.append((np.asarray(X, f32), f32(dmin), f32(dmax), np.asarray(desc, np.uint8),
                         f32(angle), skip))
        return len(self.pts) - 1

    def pair(self, u, v, octave, flips, z=10.0, dx=0.3, dy=-0.2, kf_angle=0.0, key_angle=0.0):
        """A point that projects to (u, v) with predicted level `octave`, and a key of that
        octave next to it whose descriptor is `flips` bits away.  -> (point, key)."""
        X = world_point(self.T, u, v, z)
        dmin, dmax = level_dists(dist3d(self.T, X), octave)
        d = self.rng.integers(0, 256, 32, dtype=np.uint8)
        p = self.point(X, dmin, dmax, d, kf_angle)
        k = self.key(u + dx, v + dy, octave, flipped(self.rng, d, flips), key_angle)
        return p, k

    def finish(self, n_background=0, bound_frac=0.0, clear=45.0):
        """Adds random background keys at least `clear` pixels (Chebyshev) from every placed key."""
        rng = self.rng
        placed = np.array([[k["x"][0], k["y"][0]] for k in self.keys]).reshape(-1, 2)
        bg = BP._kps(rng, n_background)
        for b in bg:
            if len(placed) and clear > 0 and \
                    (np.abs(placed - [b["x"], b["y"]]).max(1) < clear).any():
                continue
            self.key(b["x"], b["y"], b["octave"], rng.integers(0, 256, 32, dtype=np.uint8),
                     b["angle"], int(rng.random() < bound_frac))
        n, m = len(self.keys), len(self.pts)
        kps = np.concatenate(self.keys) if n else np.zeros(0, KP)
        return dict(
            kps=kps, desc=np.array(self.kdesc, np.uint8).reshape(n, 32),
            depth=np.full((H, W), 10.0, f32), tcw=self.T,
            Xw=np.array([p[0] for p in self.pts], f32).reshape(m, 3),
            min_dist=np.array([p[1] for p in self.pts], f32),
            max_dist=np.array([p[2] for p in self.pts], f32),
            pdesc=np.array([p[3] for p in self.pts], np.uint8).reshape(m, 32),
            angle=np.array([p[4] for p in self.pts], f32),
            skip=np.array([p[5] for p in self.pts], np.uint8),
            th=self.th, orb_dist=self.orb, bound=np.array(self.kbound, np.uint8), tags=self.tags)


def _sbp_round(O, which, stride, K=K):
    """The reference's two calls on kitti_sample: frame 1 at the oracle's pose against points
    back-projected from frame 0; ~20 % of the keys bound, ~10 % of the points in sAlreadyFound."""
    rng = np.random.default_rng(20 + which)
    T = MP.poses(O)
    (k0, d0, dep0), (k1, d1, dep1) = [(k[:2000], d[:2000], dep) for k, d, dep in
                                      (MP.frame(O, 0), MP.frame(O, 1))]
    Xw, md, valid, _, dmin, dmax = MP.map_points(k0, d0, dep0, T[0], rng, K=K)
    skip = (~valid) | (rng.random(len(k0)) < 0.1)
    if stride > 1:
        skip |= (np.arange(len(k0)) % stride) != 0
    bound = rng.random(len(k1)) < 0.2
    th, orb = [(10.0, 100), (3.0, 64)][which]
    return dict(kps=k1, desc=d1, depth=dep1, tcw=T[1], Xw=Xw, min_dist=dmin, max_dist=dmax,
                pdesc=md, angle=k0["angle"].astype(f32), skip=skip.astype(np.uint8), th=th,
                orb_dist=orb, bound=bound.astype(np.uint8), tags={})


def _sbp_crowded(variant):
    """More candidates in one window than k_sbp_kf lists (32), and more copies of one map point
    than that: the later copies find every listed key bound and fall to the host rescan.  The
    patch straddles a grid-cell boundary in x and in y, so GetFeaturesInArea order is not index
    order; variant "b" gives pairs of keys the same distance, so the tie falls to area order."""
    B = _Sbp(T_HAND, 10.0, 100, 30 + (variant == "b"))
    rng = B.rng
    xb, yb = 20.5 * CELL_W, 20.5 * CELL_H  # between cells 20 and 21 in both directions
    level = 2
    X = world_point(B.T, xb, yb, 12.0)
    dmin, dmax = level_dists(dist3d(B.T, X), level)   # max_dist / dist3D = 1.2^1.5
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    npatch, ncopies = 56, 44
    xs = (xb + rng.uniform(-4, 4, npatch)).astype(f32)
    ys = (yb + rng.uniform(-3, 3, npatch)).astype(f32)
    assert len(set(zip(xs.tolist(), ys.tolist()))) == npatch
    pre = set(rng.choice(npatch, 4, replace=False).tolist())  # hold a MapPoint from the start
    for i in range(npatch):
        flips = i + 1 if variant == "a" else i // 2 + 1
        k = B.key(xs[i], ys[i], level, flipped(rng, d, flips), 0.0, int(i in pre))
        B.tag("patch", k)
    for _ in range(ncopies):
        B.tag("copies", B.point(X, dmin, dmax, d))
    return B.finish(300, 0.2, clear=0.0)


def _sbp_degenerate():
    """Points the projection, the distance gate or PredictScale treat specially, each at its own
    site with a key that would match: tags `bind` / `none` list the points the reference binds
    and the points it must leave alone (asserted on the oracle's result)."""
    B = _Sbp(T_AXIS, 10.0, 100, 40)
    rng = B.rng
    t = B.T[:3, 3]
    st = iter(sites(40))

    def camera_point(xc):  # Xw with camera coordinates exactly xc (Rcw = I)
        X = (np.asarray(xc, f32) - t).astype(f32)
        zero = np.asarray(xc, f32) == 0
        assert ((X + t)[zero] == 0).all()
        return X

    def special(name, X, dmin, dmax, octave, expect, at=None):
        u, v = next(st) if at is None else at
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        p = B.point(X, dmin, dmax, d)
        B.key(u + 0.3, v - 0.2, octave, flipped(rng, d, 5))
        B.tag(name, p)
        B.tag("bind" if expect else "none", p)
        return p

    # camera z == 0: invzc = inf.  u = fx * 0 * inf + cx = NaN passes `u < minX || u > maxX`;
    # the window of a NaN centre is empty
    special("z0_nan", camera_point((0, 0, 0)), 0.0, 0.0, 0, False)
    special("z0_uinf", camera_point((1, 0, 0)), 0.0, 1e9, 0, False)
    special("z0_unan_vinf", camera_point((0, 1, 0)), 0.0, 1e9, 0, False)
    # z < 0: the reference has no depth test here, the point projects and binds
    u, v = next(st)
    X = world_point(B.T, u, v, -8.0)
    special("z_neg", X, *level_dists(dist3d(B.T, X), 3), 3, True, at=(u, v))
    # non-finite coordinates
    special("nan", np.full(3, np.nan, f32), 0.0, 1e9, 0, False)
    special("inf_x", camera_point((np.inf, 0.5, 10)), 0.0, np.inf, 0, False)
    special("inf_z", camera_point((0.5, 0.5, np.inf)), 0.0, np.inf, 0, False)
    special("ninf_z", camera_point((0.5, 0.5, -np.inf)), 0.0, np.inf, 0, False)
    # dist3D against 0.8 min_dist and 1.2 max_dist, one float apart on either side
    for name in ("min_in", "min_out", "max_in", "max_out"):
        u, v = next(st)
        X = world_point(B.T, u, v, 10.0)
        d3 = dist3d(B.T, X)
        dmin, dmax = level_dists(d3, 2)
        octave = 2
        if name.startswith("min"):
            m = f32(d3 / f32(0.8))
            while f32(f32(0.8) * m) <= d3:   # smallest min_dist with 0.8f * min_dist > dist3D
                m = np.nextafter(m, f32(np.inf))
            while f32(f32(0.8) * np.nextafter(m, f32(0))) > d3:
                m = np.nextafter(m, f32(0))
            dmin = m if name == "min_out" else np.nextafter(m, f32(0))
            dmax = max(dmax, dmin)
        else:
            m = f32(d3 / f32(1.2))
            while f32(f32(1.2) * m) >= d3:   # largest max_dist with 1.2f * max_dist < dist3D
                m = np.nextafter(m, f32(0))
            while f32(f32(1.2) * np.nextafter(m, f32(np.inf))) < d3:
                m = np.nextafter(m, f32(np.inf))
            dmax = m if name == "max_out" else np.nextafter(m, f32(np.inf))
            dmin, octave = f32(0.0), 0  # ratio ~ 1 / 1.2: level -1 or 0, clamped to 0 either way
        special(name, X, dmin, dmax, octave, name.endswith("_in"), at=(u, v))
    # PredictScale's clamps and its non-finite branch
    for name, ratio, octave, expect in (("clamp_hi", 1e4, 7, True), ("clamp_lo", 0.9, 1, True),
                                        ("max_zero", 0.0, 0, False), ("max_inf", np.inf, 0, True),
                                        ("max_nan", np.nan, 1, True)):
        u, v = next(st)
        X = world_point(B.T, u, v, 10.0)
        with np.errstate(invalid="ignore", over="ignore"):
            dmax = f32(dist3d(B.T, X) * f32(ratio))
        special(name, X, 0.0, dmax, octave, expect, at=(u, v))
    # projections within a pixel of each border: the window is clipped to the first / last cells.
    # A key past the last cell centre (round(x * invW) == 64) is in no cell: never a candidate,
    # though its descriptor is the closer one
    for name, (u, v), (kx, ky), off_grid in (
            ("left", (0.6, 100.0), (1.0, 99.5), None),
            ("right", (W - 0.6, 150.0), (1232.0, 150.5), (1236.0, 150.0)),
            ("top", (300.0, 0.6), (300.5, 1.5), None),
            ("bottom", (500.0, H - 0.6), (499.5, 370.5), (500.0, 372.5))):
        X = world_point(B.T, u, v, 10.0)
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        p = B.point(X, *level_dists(dist3d(B.T, X), 1), d)
        B.key(kx, ky, 1, flipped(rng, d, 9))
        if off_grid:
            B.tag("off_grid", B.key(off_grid[0], off_grid[1], 1, flipped(rng, d, 1)))
        B.tag(name, p)
        B.tag("bind", p)
    # a point in sAlreadyFound that would bind otherwise
    u, v = next(st)
    p, _ = B.pair(u, v, 2, 4)
    B.pts[p] = B.pts[p][:5] + (1,)
    B.tag("none", p)
    return B.finish(250, 0.0)


def _sbp_orbdist_edge(th, orb):
    """Isolated pairs at Hamming distance ORBdist - 1, ORBdist and ORBdist + 1."""
    B = _Sbp(T_HAND, th, orb, 50 + orb)
    for (u, v), delta, octave in zip(sites(9), (-1, 0, 1) * 3, (0, 0, 0, 2, 2, 2, 5, 5, 5)):
        p, _ = B.pair(u, v, octave, orb + delta)
        B.tag("bind" if delta <= 0 else "none", p)
    return B.finish(250, 0.1)


def _sbp_rotation(variant):
    """The rotation histogram.  "a": a common rotation, a third of the keyframe angles perturbed;
    "b": twelve bins of three matches each (rot * 1/30 reaches bins 0..12 only), so
    ComputeThreeMaxima keeps the first three bins."""
    B = _Sbp(T_HAND, 10.0, 100, 60 + (variant == "b"))
    rng = B.rng
    if variant == "a":
        for i, (u, v) in enumerate(sites(60)):
            key_angle = rng.uniform(0, 360)
            kf_angle = (key_angle + 20 + rng.normal(0, 1.0)) % 360
            if i % 3 == 0:
                kf_angle = (key_angle + rng.uniform(60, 300)) % 360
                B.tag("perturbed", i)
            B.pair(u, v, int(rng.integers(0, 8)), int(rng.integers(0, 30)), kf_angle=kf_angle,
                   key_angle=key_angle)
    else:
        for i, (u, v) in enumerate(sites(36)):
            B.pair(u, v, int(rng.integers(0, 8)), 3, kf_angle=10.0 + 30.0 * (i % 12),
                   key_angle=10.0)
    return B.finish(200, 0.0)


def _sbp_sizes(m, empty_frame=False):
    """m points (a workgroup of k_sbp_kf holds four), or a current frame without keys."""
    B = _Sbp(T_HAND, 10.0, 100, 70)
    for (u, v) in sites(m):
        B.pair(u, v, 2, 6)
    if empty_frame:
        B.keys, B.kdesc, B.kbound = [], [], []
        return B.finish(0)
    return B.finish(150, 0.1)


SBP_CASES = ["round1", "round2", "crowded_a", "crowded_b", "degenerate", "orbdist_edge_100",
             "orbdist_edge_64", "rotation_a", "rotation_b", "m0", "m1", "m5", "empty_frame"]
SBP_KITTI = ("round1", "round2")


def sbp_case(O, name, stride=1, K=K):
    """Inputs of one named SearchByProjection(F, KF) case (cached: callers must not write to
    them).  stride > 1 keeps every stride-th point of the kitti cases; K is the camera the kitti
    cases' points are back-projected with (the hand-built cases are KITTI's)."""
    assert K == MP.K or name in SBP_KITTI, name
    key = ("sbp", name, stride, K)
    if key not in _CACHE:
        if name in SBP_KITTI:
            c = _sbp_round(O, SBP_KITTI.index(name), stride, K)
        elif name.startswith("crowded_"):
            c = _sbp_crowded(name[-1])
        elif name == "degenerate":
            c = _sbp_degenerate()
        elif name == "orbdist_edge_100":
            c = _sbp_orbdist_edge(10.0, 100)
        elif name == "orbdist_edge_64":
            c = _sbp_orbdist_edge(3.0, 64)
        elif name.startswith("rotation_"):
            c = _sbp_rotation(name[-1])
        elif name == "empty_frame":
            c = _sbp_sizes(5, True)
        elif name in ("m0", "m1", "m5"):
            c = _sbp_sizes(int(name[1:]))
        else:
            raise KeyError(name)
        _CACHE[key] = c
    return _CACHE[key]


def sbp_args(c):
    """Positional arguments shared by Context.search_by_projection_keyframe and the oracle's."""
    return (c["kps"], c["desc"], c["depth"], c["tcw"], c["Xw"], c["min_dist"], c["max_dist"],
            c["pdesc"], c["angle"], c["skip"], c["th"], c["orb_dist"], c["bound"])


# ------------------------------------------------------------------ SearchForTriangulation
T1_HAND = np.eye(4, dtype=f32)
T2_HAND = pose(rot_y(0.03), (0.3, -0.05, 1.2))  # forward motion: the epipole is inside the image


def _keyframe(kps, desc, uR, has_mp, fv, T):
    n = len(kps)
    return dict(kps=np.asarray(kps, KP), desc=np.asarray(desc, np.uint8).reshape(n, 32),
                uR=np.asarray(uR, f32), has_mp=np.asarray(has_mp, np.uint8),
                fv=fv, Tcw=np.asarray(T, f32))


def _kp(x, y, octave):
    assert 0 <= x < W and 0 <= y < H, (x, y)
    k = np.zeros(1, KP)
    k["x"], k["y"], k["octave"], k["size"] = x, y, octave, 31
    return k


def epipolar_line(F, x1, y1):
    """(a, b, c) of the keyframe-2 line of keyframe-1 pixel (x1, y1), in float64 from the float F12."""
    F = F.astype(np.float64)
    return (x1 * F[0, 0] + y1 * F[1, 0] + F[2, 0], x1 * F[0, 1] + y1 * F[1, 1] + F[2, 1],
            x1 * F[0, 2] + y1 * F[1, 2] + F[2, 2])


def epipole(T1, T2, K=K):
    """Projection of keyframe 1's centre into keyframe 2 (float64)."""
    T1 = T1.astype(np.float64)
    T2 = T2.astype(np.float64)
    Ow = -T1[:3, :3].T @ T1[:3, 3]
    c = T2[:3, :3] @ Ow + T2[:3, 3]
    return K[0] * c[0] / c[2] + K[2], K[1] * c[1] / c[2] + K[3]


def _project2(x1, y1, z, T2=None):
    """Keyframe-2 pixel of the point at depth z on keyframe-1 pixel (x1, y1)'s ray (T1 = I)."""
    X = np.array([(x1 - K[2]) * z / K[0], (y1 - K[3]) * z / K[1], z])
    T2 = (T2_HAND if T2 is None else T2).astype(np.float64)
    c = T2[:3, :3] @ X + T2[:3, 3]
    return K[0] * c[0] / c[2] + K[2], K[1] * c[1] / c[2] + K[3]


class _Sft:
    """Builder of a hand-built pair of keyframes: every query gets a vocabulary node of its own."""

    def __init__(self, seed, T1=T1_HAND, T2=T2_HAND):
        self.rng = np.random.default_rng(seed)
        self.T1, self.T2 = T1, T2
        self.F = compute_f12(T1, T2)
        self.k = ([], [])
        self.d = ([], [])
        self.u = ([], [])
        self.has = ([], [])
        self.node = ([], [])
        self.tags = {}
        self.next_node = 100

    def tag(self, name, v):
        self.tags.setdefault(name, []).append(v)

    def add(self, side, x, y, octave, desc, node, stereo=True, has_mp=0):
        self.k[side].append(_kp(x, y, octave))
        self.d[side].append(np.asarray(desc, np.uint8))
        self.u[side].append(f32(x - 3.0) if stereo else f32(-1))
        self.has[side].append(has_mp)
        self.node[side].append(node)
        return len(self.k[side]) - 1

    def query(self, x1, y1, octave=0, stereo=True):
        """A keyframe-1 feature in a fresh node.  -> (idx1, node, descriptor)."""
        node = self.next_node
        self.next_node += 7
        d = self.rng.integers(0, 256, 32, dtype=np.uint8)
        return self.add(0, x1, y1, octave, d, node, stereo), node, d

    def on_line(self, x1, y1, z=15.0, perp=0.0, at=None):
        """A keyframe-2 pixel `perp` pixels from (x1, y1)'s epipolar line, next to the image of the
        depth-z point of the ray (or to `at`)."""
        a, b, c = epipolar_line(self.F, float(f32(x1)), float(f32(y1)))
        px, py = _project2(x1, y1, z) if at is None else at
        s = (a * px + b * py + c) / (a * a + b * b)
        px, py = px - s * a, py - s * b
        n = np.hypot(a, b)
        return px + perp * a / n, py + perp * b / n

    def finish(self, shuffle=False):
        out = []
        srng = np.random.default_rng(5) if shuffle else None
        for side, T in ((0, self.T1), (1, self.T2)):
            n = len(self.k[side])
            kps = np.concatenate(self.k[side]) if n else np.zeros(0, KP)
            fv = BP.feature_vector(np.array(self.node[side], np.int64), srng)
            out.append(_keyframe(kps, np.array(self.d[side], np.uint8), self.u[side],
                                 self.has[side], fv, T))
        return dict(kf1=out[0], kf2s=[out[1]], tags=self.tags)


def _sft_kitti(O, stride, K=K, BF=BF):
    """kitti_sample frame 0 against frames 1 and 2 in one call: poses from the oracle tracker,
    mvuRight from the oracle's frame grid, FeatureVectors from the test vocabulary; about half of
    the keys hold a MapPoint and 30 % of the rest are monocular (uR = -1)."""
    rng = np.random.default_rng(80)
    T = MP.poses(O)
    voc = O.Vocabulary(VOC)
    kfs = []
    for i in range(3):
        k, d, dep = MP.frame(O, i)
        k, d = k[:2000], d[:2000]
        uR = O.frame_stereo_grid(k, dep, K, BF)[0].copy()
        has = rng.random(len(k)) < 0.5
        uR[(~has) & (rng.random(len(k)) < 0.3)] = -1
        # the keys around the focus of expansion: free and monocular, so the epipole test acts
        ex, ey = epipole(T[0], T[max(i, 1)], K)
        near = np.hypot(k["x"] - ex, k["y"] - ey) < 30
        has[near] = False
        uR[near] = -1
        if i == 0 and stride > 1:
            has |= (np.arange(len(k)) % stride) != 0
        kfs.append(_keyframe(k, d, uR, has, voc.transform(d, 4)["fv"], T[i]))
    return dict(kf1=kfs[0], kf2s=kfs[1:], tags={})


def _sft_th_low_edge():
    """Keyframe-2 features on the query's epipolar line at Hamming distance exactly 50 and 51
    (TH_LOW), and features of a close descriptor at 0.5 and 2 times sqrt(3.84 sigma2[octave]) from
    the line, on either side."""
    B = _Sft(90)
    rng = B.rng
    st = iter(sites(40, x0=150.0, dx=60.0, cols=14))
    for octave in (0, 3, 7):
        for dist, expect in ((50, True), (51, False)):
            x1, y1 = next(st)
            i1, node, d = B.query(x1, y1, int(rng.integers(0, 8)))
            x2, y2 = B.on_line(x1, y1)
            i2 = B.add(1, x2, y2, octave, flipped(rng, d, dist), node)
            B.tag("match" if expect else "none", (i1, i2))
        sigma = 1.2 ** octave
        for mult, expect in ((0.5, True), (2.0, False), (-0.5, True), (-2.0, False)):
            x1, y1 = next(st)
            i1, node, d = B.query(x1, y1, int(rng.integers(0, 8)))
            x2, y2 = B.on_line(x1, y1, perp=mult * np.sqrt(3.84) * sigma)
            i2 = B.add(1, x2, y2, octave, flipped(rng, d, 12), node)
            B.tag("match" if expect else "none", (i1, i2))
    return B.finish()


def _sft_ties():
    """Equal distances inside one node, all on the line: `dist > bestDist` lets a later feature of
    the same distance replace the earlier one, so the last of the equal best wins."""
    B = _Sft(91)
    rng = B.rng
    st = iter(sites(12, x0=150.0, dx=80.0, cols=10))
    for dists, winner in (((0, 0), 1), ((10, 10), 1), ((10, 10, 12), 1), ((12, 10, 10, 10), 3),
                          ((50, 50), 1), ((7, 7, 6, 7), 2)):
        x1, y1 = next(st)
        i1, node, d = B.query(x1, y1, 1)
        idx2 = []
        for j, dist in enumerate(dists):
            x2, y2 = B.on_line(x1, y1, z=12.0 + 2.0 * j)
            idx2.append(B.add(1, x2, y2, 1, flipped(rng, d, dist), node))
        B.tag("winner", (i1, idx2[winner]))
    return B.finish()


def _sft_epipole():
    """The mono / mono exclusion around the epipole, distex^2 + distey^2 < 100 * scale[octave]:
    candidates on the query's line (every epipolar line passes through the epipole) inside and
    outside that radius, and inside it with either feature stereo, where the test does not act."""
    B = _Sft(92)
    rng = B.rng
    ex, ey = epipole(B.T1, B.T2)
    assert 50 < ex < W - 50 and 50 < ey < H - 50
    st = iter(sites(16, x0=150.0, dx=60.0, cols=14))
    for octave in (0, 4):
        rad = np.sqrt(100 * 1.2 ** octave)
        for r, s1, s2, expect in ((0.5 * rad, False, False, False), (1.3 * rad, False, False, True),
                                  (0.5 * rad, True, False, True), (0.5 * rad, False, True, True),
                                  (0.96 * rad, False, False, False), (1.04 * rad, False, False, True)):
            x1, y1 = next(st)
            i1, node, d = B.query(x1, y1, 2, stereo=s1)
            a, b, _ = epipolar_line(B.F, float(f32(x1)), float(f32(y1)))
            n = np.hypot(a, b)
            x2, y2 = B.on_line(x1, y1, at=(ex + r * b / n, ey - r * a / n))  # along the line
            i2 = B.add(1, x2, y2, octave, flipped(rng, d, 8), node, stereo=s2)
            B.tag("match" if expect else "none", (i1, i2))
    return B.finish()


def _two_view(seed, n1, n2, node1, node2, T2=T2_HAND, has1=0.3, has2=0.3, n_free1=None):
    """Random 3D points seen by both hand poses: keyframe 2's first min(n1, n2) features are
    keyframe 1's (pixel noise below a pixel, descriptors up to 60 bits away), 30 % monocular."""
    rng = np.random.default_rng(seed)

    def view(n):
        k = np.zeros(n, KP)
        k["x"] = rng.uniform(80, W - 80, n).astype(f32)
        k["y"] = rng.uniform(60, H - 60, n).astype(f32)
        k["octave"] = rng.integers(0, 8, n)
        k["size"] = 31
        return k, rng.integers(0, 256, (n, 32), dtype=np.uint8)
    k1, d1 = view(n1)
    k2, d2 = view(n2)
    for i in range(min(n1, n2)):
        if np.array_equal(T2, T1_HAND):
            x2, y2 = float(k1["x"][i]), float(k1["y"][i])
        else:
            x2, y2 = _project2(float(k1["x"][i]), float(k1["y"][i]), rng.uniform(8, 40), T2)
        x2, y2 = x2 + rng.normal(0, 0.6), y2 + rng.normal(0, 0.6)
        if 1 <= x2 < W - 1 and 1 <= y2 < H - 1:
            k2["x"][i], k2["y"][i] = x2, y2
            k2["octave"][i] = k1["octave"][i]
            d2[i] = flipped(rng, d1[i], rng.integers(0, 60))
    u1 = np.where(rng.random(n1) < 0.3, -1, k1["x"] - 4).astype(f32)
    u2 = np.where(rng.random(n2) < 0.3, -1, k2["x"] - 4).astype(f32)
    h1 = rng.random(n1) < has1
    if n_free1 is not None:  # exactly n_free1 keyframe-1 features without a MapPoint
        h1[:] = True
        h1[rng.choice(n1, n_free1, replace=False)] = False
    h2 = rng.random(n2) < has2
    fv1 = BP.feature_vector(np.asarray(node1(rng, n1), np.int64))
    fv2 = BP.feature_vector(np.asarray(node2(rng, n2), np.int64))
    return dict(kf1=_keyframe(k1, d1, u1, h1, fv1, T1_HAND),
                kf2s=[_keyframe(k2, d2, u2, h2, fv2, T2)], tags={})


def _one(rng, n):
    return np.full(n, 42)


SFT_CASES = ["kitti", "th_low_edge", "ties", "epipole", "den_zero", "one_node", "disjoint",
             "nq_257", "three_pairs", "empty_kf1", "empty_kf2"]


def sft_case(O, name, stride=1, K=K, BF=BF):
    """Inputs of one named SearchForTriangulation case (cached: callers must not write to them):
    dict(kf1, kf2s, tags).  stride > 1 keeps every stride-th query feature of the kitti case; K, BF
    are the camera of the kitti case (the hand-built cases are KITTI's)."""
    assert (K, BF) == (MP.K, MP.BF) or name == "kitti", name
    key = ("sft", name, stride, K, BF)
    if key in _CACHE:
        return _CACHE[key]
    if name == "kitti":
        c = _sft_kitti(O, stride, K, BF)
    elif name == "th_low_edge":
        c = _sft_th_low_edge()
    elif name == "ties":
        c = _sft_ties()
    elif name == "epipole":
        c = _sft_epipole()
    elif name == "den_zero":      # T1 == T2: F12 = 0, a = b = 0 for every query
        c = _two_view(93, 120, 120, _one, _one, T2=T1_HAND)
    elif name == "one_node":
        c = _two_view(94, 300, 300, _one, _one)
    elif name == "disjoint":      # even nodes against odd nodes
        c = _two_view(95, 200, 200, lambda r, n: 2 * r.integers(0, 20, n),
                      lambda r, n: 2 * r.integers(0, 20, n) + 1)
    elif name == "nq_257":        # one query past a 256-thread workgroup
        c = _two_view(96, 300, 280, _one, _one, n_free1=257)
    elif name == "three_pairs":   # per-pair feature tables and flags of different sizes
        mod6 = lambda r, n: np.arange(n) % 6   # noqa: E731  (a feature and its copy share a node)
        a = _two_view(97, 260, 300, mod6, mod6)
        b = _two_view(97, 260, 90, mod6, lambda r, n: np.arange(n) % 6 + 6 * (np.arange(n) % 5 == 0))
        e = _two_view(97, 260, 180, mod6, lambda r, n: np.arange(n) % 3,
                      T2=pose(rot_y(-0.02), (-0.4, 0.02, 0.9)))
        c = dict(kf1=a["kf1"], kf2s=[a["kf2s"][0], b["kf2s"][0], e["kf2s"][0]], tags={})
    elif name == "empty_kf1":
        c = _two_view(98, 0, 50, _one, _one)
    elif name == "empty_kf2":
        c = _two_view(99, 50, 0, _one, _one)
    else:
        raise KeyError(name)
    _CACHE[key] = c
    return c
