"""The oracle's two vocabulary-path matchers against pure-Python restatements of the reference, on
the cases of reloc_problems (CPU only):

  * ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)
    (ORBmatcher.cc:2104-2231) with Frame::GetFeaturesInArea (Frame.cc:711-758), PosInGrid
    (Frame.cc:765-775) and MapPoint::PredictScale (MapPoint.cc:402-417);
  * ORBmatcher::SearchForTriangulation (ORBmatcher.cc:1032-1131) with CheckDistEpipolarLine
    (ORBmatcher.cc:513-530) and LocalMapping::ComputeF12.

Bindings and counts are compared exactly.  The restatements compute in numpy float32 in the
reference's operation order (products of cv::Mat expressions accumulate in double and round to
float once, as DESIGN.md section 2 pins them), so comparisons near a threshold agree.  Each case
also asserts the property it exists for, from the inputs, the restatement or the oracle's result;
test_gpu_reloc_match.py then holds the GPU to the oracle on the same cases."""
import math

import numpy as np
import pytest

import match_problems as MP
import reloc_problems as RP

f32 = np.float32
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
HISTO_LENGTH, TH_LOW = 30, 50
COLS, ROWS = 64, 48
_RESULTS = {}


def hamming(a, b):
    return int(POP[np.bitwise_xor(a, b)].sum())


def c_round(v):
    """C's round(): halves away from zero."""
    v = float(v)
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def xform(T, x):
    """Rcw * x + tcw: the product accumulated in double and rounded once, the sum in float."""
    y = np.zeros(3, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            s = np.float64(0.0)
            for k in range(3):
                s = s + np.float64(T[r, k]) * np.float64(x[k])
            y[r] = f32(s) + T[r, 3]
    return y


def cam_centre(T):
    Ow = np.zeros(3, f32)
    for r in range(3):
        s = 0.0
        for k in range(3):
            s += float(T[k, r]) * float(T[k, 3])
        Ow[r] = -f32(s)
    return Ow


def three_maxima(hist):
    """ORBmatcher::ComputeThreeMaxima."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i in range(HISTO_LENGTH):
        s = len(hist[i])
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif max3 < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


class Grid:
    """Frame::AssignFeaturesToGrid / PosInGrid and GetFeaturesInArea over [0, W] x [0, H]."""

    def __init__(self, kps):
        self.kps = kps
        self.minX, self.minY = f32(0), f32(0)
        self.invW = f32(COLS) / f32(f32(RP.W) - self.minX)
        self.invH = f32(ROWS) / f32(f32(RP.H) - self.minY)
        self.cells = {}
        for i in range(len(kps)):
            px = c_round(f32(kps["x"][i] - self.minX) * self.invW)
            py = c_round(f32(kps["y"][i] - self.minY) * self.invH)
            if px < 0 or px >= COLS or py < 0 or py >= ROWS:
                continue
            self.cells.setdefault((px, py), []).append(i)

    def area(self, x, y, r, min_level, max_level):
        # a non-finite centre: the reference's float -> int conversions give INT_MIN on x86 and an
        # empty cell range (pinned, oracle/match_ref.cpp)
        if not (np.isfinite(x) and np.isfinite(y)):
            return []
        x0 = max(0, int(math.floor(f32(f32(x - self.minX) - r) * self.invW)))
        if x0 >= COLS:
            return []
        x1 = min(COLS - 1, int(math.ceil(f32(f32(x - self.minX) + r) * self.invW)))
        if x1 < 0:
            return []
        y0 = max(0, int(math.floor(f32(f32(y - self.minY) - r) * self.invH)))
        if y0 >= ROWS:
            return []
        y1 = min(ROWS - 1, int(math.ceil(f32(f32(y - self.minY) + r) * self.invH)))
        if y1 < 0:
            return []
        check = min_level > 0 or max_level >= 0
        out = []
        kx, ky, ko = self.kps["x"], self.kps["y"], self.kps["octave"]
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                for k in self.cells.get((ix, iy), ()):
                    if check:
                        if ko[k] < min_level:
                            continue
                        if max_level >= 0 and ko[k] > max_level:
                            continue
                    if abs(f32(kx[k] - x)) < r and abs(f32(ky[k] - y)) < r:
                        out.append(k)
        return out


def predict_scale(max_dist, dist, log_scale, nlevels):
    """MapPoint::PredictScale(currentDist, Frame*); a non-finite level converts to INT_MIN."""
    with np.errstate(all="ignore"):
        ratio = f32(max_dist) / f32(dist)
        if ratio > 0 and np.isfinite(ratio):
            ls = f32(math.log(float(ratio))) / log_scale
        elif ratio == 0:
            ls = f32(-np.inf)
        else:
            ls = f32(np.log(np.float64(ratio))) / log_scale  # inf, NaN, negative
    n = int(math.ceil(ls)) if np.isfinite(ls) else -2 ** 31
    if n < 0:
        n = 0
    elif n >= nlevels:
        n = nlevels - 1
    return n


def restate_sbp(c, scale):
    """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist).  Returns dict(match,
    nmatches) and what the cases assert: `bound_before_hist` (matches before the rotation
    histogram), `ranks` (per bound point, the rank of its key among the window's candidates that
    held no MapPoint when the call started, by distance then area order) and `n_exhausted` (points
    that found the 32 best of more than 32 such candidates all bound by earlier points)."""
    kps, desc, T = c["kps"], c["desc"], c["tcw"].astype(f32)
    fx, fy, cx, cy = [f32(v) for v in RP.K]
    G = Grid(kps)
    maxX, maxY = f32(RP.W), f32(RP.H)
    log_scale = f32(math.log(float(f32(scale[1]))))
    Ow = cam_centre(T)
    mp_of = np.where(c["bound"] != 0, -2, -1).astype(np.int64)  # -2: a MapPoint from before
    start_bound = c["bound"] != 0
    hist = [[] for _ in range(HISTO_LENGTH)]
    factor = f32(1.0) / f32(HISTO_LENGTH)
    th, orb = f32(c["th"]), int(c["orb_dist"])
    nmatches, ranks, n_exhausted = 0, [], 0
    for i in range(len(c["skip"])):
        if c["skip"][i]:
            continue
        pos = c["Xw"][i]
        xc = xform(T, pos)
        with np.errstate(all="ignore"):
            invzc = f32(np.float64(1.0) / np.float64(xc[2]))
            u = f32(f32(fx * xc[0]) * invzc) + cx
            v = f32(f32(fy * xc[1]) * invzc) + cy
            if u < G.minX or u > maxX:
                continue
            if v < G.minY or v > maxY:
                continue
            s = np.float64(0.0)
            for k in range(3):
                d = f32(pos[k] - Ow[k])
                s = s + np.float64(d) * np.float64(d)
            dist3D = f32(np.sqrt(s))
            max_distance = f32(1.2) * c["max_dist"][i]
            min_distance = f32(0.8) * c["min_dist"][i]
            if dist3D < min_distance or dist3D > max_distance:
                continue
        level = predict_scale(c["max_dist"][i], dist3D, log_scale, len(scale))
        radius = th * f32(scale[level])
        idx = G.area(u, v, radius, level - 1, level + 1)
        if not idx:
            continue
        best_dist, best = 256, -1
        cands = []
        for order, i2 in enumerate(idx):
            dist = None
            if not start_bound[i2]:
                dist = hamming(c["pdesc"][i], desc[i2])
                cands.append((dist, order, i2))
            if mp_of[i2] != -1:
                continue
            if dist < best_dist:
                best_dist, best = dist, i2
        cands.sort()
        if len(cands) > 32 and all(mp_of[k] != -1 for _, _, k in cands[:32]):
            n_exhausted += 1
        if best_dist <= orb:
            mp_of[best] = i
            nmatches += 1
            ranks.append([k for _, _, k in cands].index(best))
            rot = f32(c["angle"][i]) - f32(kps["angle"][best])
            if rot < 0.0:
                rot = rot + f32(360.0)
            b = c_round(rot * factor)
            if b == HISTO_LENGTH:
                b = 0
            assert 0 <= b < HISTO_LENGTH
            hist[b].append(best)
    before = nmatches
    keep = three_maxima(hist)
    for b in range(HISTO_LENGTH):
        if b in keep:
            continue
        for k in hist[b]:
            mp_of[k] = -1
            nmatches -= 1
    match = np.where(mp_of >= 0, mp_of, -1).astype(np.int32)
    return dict(match=match, nmatches=nmatches, bound_before_hist=before, ranks=ranks,
                n_exhausted=n_exhausted)


def check_epipolar(kp1, kp2, F, sigma2):
    """ORBmatcher::CheckDistEpipolarLine; F row-major float32, sigma2 = mvLevelSigma2[octave]."""
    x1, y1, x2, y2 = f32(kp1["x"]), f32(kp1["y"]), f32(kp2["x"]), f32(kp2["y"])
    a = f32(f32(x1 * F[0, 0]) + f32(y1 * F[1, 0])) + F[2, 0]
    b = f32(f32(x1 * F[0, 1]) + f32(y1 * F[1, 1])) + F[2, 1]
    c = f32(f32(x1 * F[0, 2]) + f32(y1 * F[1, 2])) + F[2, 2]
    num = f32(f32(a * x2) + f32(b * y2)) + c
    den = f32(a * a) + f32(b * b)
    if den == 0:
        return False
    dsqr = f32(num * num) / den
    return float(dsqr) < 3.84 * float(sigma2)


def restate_sft(kf1, kf2, scale):
    """ComputeF12 + SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, false).  Returns
    dict(match12, nmatches, F12) and the counts the cases assert: `nq` (keyframe-1 features without
    a MapPoint in a node both keyframes hold) and `epipole_rejected` (candidates the mono / mono
    epipole test drops)."""
    scale = np.asarray(scale, f32)
    fx, fy, cx, cy = [f32(v) for v in RP.K]
    T1, T2 = kf1["Tcw"].astype(f32), kf2["Tcw"].astype(f32)
    F = RP.compute_f12(T1, T2)
    C2 = xform(T2, cam_centre(T1))
    with np.errstate(all="ignore"):
        invz = f32(1.0) / C2[2]
        ex = f32(f32(fx * C2[0]) * invz) + cx
        ey = f32(f32(fy * C2[1]) * invz) + cy
    n1 = len(kf1["kps"])
    m12 = np.full(n1, -1, np.int32)
    nmatches = nq = rejected = 0
    node1, start1, feat1 = kf1["fv"]
    node2, start2, feat2 = kf2["fv"]
    at2 = {int(n): j for j, n in enumerate(node2)}
    for a, nid in enumerate(node1):  # the merge of two ascending maps visits the common ids
        if int(nid) not in at2:
            continue
        b = at2[int(nid)]
        list2 = feat2[start2[b]:start2[b + 1]]
        for idx1 in feat1[start1[a]:start1[a + 1]]:
            if kf1["has_mp"][idx1]:
                continue
            nq += 1
            stereo1 = kf1["uR"][idx1] >= 0
            kp1 = kf1["kps"][idx1]
            dists = POP[np.bitwise_xor(kf2["desc"][list2], kf1["desc"][idx1])].sum(1) \
                if len(list2) else []
            best_dist, best = TH_LOW, -1
            for idx2, dist in zip(list2, dists):
                if kf2["has_mp"][idx2]:
                    continue
                stereo2 = kf2["uR"][idx2] >= 0
                if dist > TH_LOW or dist > best_dist:
                    continue
                kp2 = kf2["kps"][idx2]
                if not stereo1 and not stereo2:
                    with np.errstate(all="ignore"):
                        distex, distey = ex - f32(kp2["x"]), ey - f32(kp2["y"])
                        if f32(distex * distex) + f32(distey * distey) < \
                                f32(100) * scale[kp2["octave"]]:
                            rejected += 1
                            continue
                s = scale[kp2["octave"]]
                if check_epipolar(kp1, kp2, F, f32(s * s)):
                    best, best_dist = int(idx2), int(dist)
            if best >= 0:
                m12[idx1] = best
                nmatches += 1
    return dict(match12=m12, nmatches=nmatches, F12=F, nq=nq, epipole_rejected=rejected)


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def scale(oracle_mod):
    return MP.scale_factors(oracle_mod)


def _sbp(O, scale, name, stride=1):
    """(case, oracle result, restatement), computed once."""
    key = ("sbp", name, stride)
    if key not in _RESULTS:
        c = RP.sbp_case(O, name, stride)
        nm, m = O.search_by_projection_keyframe(*RP.sbp_args(c), RP.K, RP.BF, scale)
        _RESULTS[key] = (c, (nm, m), restate_sbp(c, scale))
    return _RESULTS[key]


def _sft(O, scale, name, stride=1):
    key = ("sft", name, stride)
    if key not in _RESULTS:
        c = RP.sft_case(O, name, stride)
        orc = O.search_for_triangulation(c["kf1"], c["kf2s"], RP.K, RP.BF, scale)
        _RESULTS[key] = (c, orc, [restate_sft(c["kf1"], k2, scale) for k2 in c["kf2s"]])
    return _RESULTS[key]


def _point_of(match, n_points):
    """key bound to each point (-1: none) from match[key] = point."""
    out = np.full(n_points, -1, np.int64)
    for k, p in enumerate(match):
        if p >= 0:
            out[p] = k
    return out


# ------------------------------------------------------------------ SearchByProjection(F, KF)
@pytest.mark.parametrize("name", RP.SBP_CASES)
def test_sbp_oracle_matches_restatement(oracle_mod, scale, name):
    c, (nm, m), r = _sbp(oracle_mod, scale, name, 3 if name in RP.SBP_KITTI else 1)
    assert len(m) == len(c["kps"])
    assert np.array_equal(m, r["match"]), np.nonzero(m != r["match"])[0][:10]
    assert nm == r["nmatches"] == int((m >= 0).sum())
    # a key that held a MapPoint is never bound again, a skipped point never binds
    assert (m[c["bound"] != 0] == -1).all()
    assert not (c["skip"][m[m >= 0]] != 0).any()


@pytest.mark.parametrize("name", RP.SBP_KITTI)
def test_sbp_kitti_rounds_find_matches(oracle_mod, scale, name):
    c = RP.sbp_case(oracle_mod, name)
    nm, m = oracle_mod.search_by_projection_keyframe(*RP.sbp_args(c), RP.K, RP.BF, scale)
    assert nm > 50, nm


@pytest.mark.parametrize("name", ["crowded_a", "crowded_b"])
def test_sbp_crowded_needs_more_than_the_listed_candidates(oracle_mod, scale, name):
    c, (nm, m), r = _sbp(oracle_mod, scale, name)
    t = c["tags"]
    assert len(t["patch"]) >= 48 and len(t["copies"]) >= 40
    # one octave, distinct positions within a few pixels, on both sides of a cell boundary in x
    k = c["kps"][t["patch"]]
    assert len(set(k["octave"].tolist())) == 1
    assert len({(x, y) for x, y in zip(k["x"].tolist(), k["y"].tolist())}) == len(k)
    assert np.ptp(k["x"]) < 10 and np.ptp(k["y"]) < 10
    cells = {c_round(f32(x) * (f32(64) / f32(RP.W))) for x in k["x"]}
    assert len(cells) == 2
    # every copy binds a patch key, all below ORBdist
    bound_to = _point_of(m, len(c["skip"]))
    assert (bound_to[t["copies"]] >= 0).all()
    assert set(bound_to[t["copies"]].tolist()) <= set(t["patch"])
    # the property: some point's key is not among the 32 best candidates of its window
    assert max(r["ranks"]) >= 32, max(r["ranks"])
    assert r["n_exhausted"] > 0
    if name == "crowded_b":  # equal distances: the pair's first key in area order goes first
        d = [hamming(c["pdesc"][t["copies"][0]], c["desc"][j]) for j in t["patch"]]
        assert len(set(d)) < len(d)


def test_sbp_degenerate_points(oracle_mod, scale):
    c, (nm, m), r = _sbp(oracle_mod, scale, "degenerate")
    t = c["tags"]
    bound_to = _point_of(m, len(c["skip"]))
    for name in ("z0_nan", "z0_uinf", "z0_unan_vinf", "z_neg", "nan", "inf_x", "inf_z", "ninf_z",
                 "min_in", "min_out", "max_in", "max_out", "clamp_hi", "clamp_lo", "max_zero",
                 "max_inf", "max_nan", "left", "right", "top", "bottom"):
        assert len(t[name]) == 1
    assert (bound_to[t["bind"]] >= 0).all(), [p for p in t["bind"] if bound_to[p] < 0]
    assert (bound_to[t["none"]] < 0).all(), [p for p in t["none"] if bound_to[p] >= 0]
    assert (m[t["off_grid"]] == -1).all()
    assert nm == len(t["bind"])
    # the z == 0 point projects to NaN, which passes the image-bounds test
    xc = xform(c["tcw"], c["Xw"][t["z0_nan"][0]])
    assert xc[2] == 0 and xc[0] == 0 and xc[1] == 0
    assert xform(c["tcw"], c["Xw"][t["z_neg"][0]])[2] < 0


@pytest.mark.parametrize("name", ["orbdist_edge_100", "orbdist_edge_64"])
def test_sbp_orbdist_edge(oracle_mod, scale, name):
    c, (nm, m), r = _sbp(oracle_mod, scale, name)
    t = c["tags"]
    bound_to = _point_of(m, len(c["skip"]))
    orb = c["orb_dist"]
    assert (bound_to[t["bind"]] >= 0).all() and (bound_to[t["none"]] < 0).all()
    d = sorted(hamming(c["pdesc"][p], c["desc"][bound_to[p]]) for p in t["bind"])
    assert d == [orb - 1] * 3 + [orb] * 3
    assert len(t["none"]) == 3 and nm == 6


def test_sbp_rotation_histogram(oracle_mod, scale):
    c, (nm, m), r = _sbp(oracle_mod, scale, "rotation_a")
    assert r["bound_before_hist"] == len(c["skip"]) == 60
    assert 0 < nm < r["bound_before_hist"]  # the histogram removed some
    bound_to = _point_of(m, 60)
    assert (bound_to[c["tags"]["perturbed"]] < 0).sum() > 10
    c, (nm, m), r = _sbp(oracle_mod, scale, "rotation_b")
    assert r["bound_before_hist"] == 36 and nm == 9  # twelve equal bins: the first three stay
    bound_to = _point_of(m, 36)
    assert all((bound_to[i] >= 0) == (i % 12 < 3) for i in range(36))


def test_sbp_sizes(oracle_mod, scale):
    for name, want in (("m0", 0), ("m1", 1), ("m5", 5), ("empty_frame", 0)):
        c, (nm, m), r = _sbp(oracle_mod, scale, name)
        assert nm == want and len(m) == len(c["kps"])
    assert len(RP.sbp_case(oracle_mod, "empty_frame")["kps"]) == 0
    assert len(RP.sbp_case(oracle_mod, "empty_frame")["skip"]) == 5


# ------------------------------------------------------------------ SearchForTriangulation
@pytest.mark.parametrize("name", RP.SFT_CASES)
def test_sft_oracle_matches_restatement(oracle_mod, scale, name):
    c, (nm, m12, F), rs = _sft(oracle_mod, scale, name, 4 if name == "kitti" else 1)
    assert m12.shape == (len(c["kf2s"]), len(c["kf1"]["kps"]))
    for p, r in enumerate(rs):
        assert np.array_equal(F[p].view(np.uint32), r["F12"].view(np.uint32)), (p, F[p], r["F12"])
        assert np.array_equal(m12[p], r["match12"]), (p, np.nonzero(m12[p] != r["match12"])[0][:10])
        assert nm[p] == r["nmatches"] == int((m12[p] >= 0).sum())
        # a match joins two features without a MapPoint
        i1 = np.nonzero(m12[p] >= 0)[0]
        assert not c["kf1"]["has_mp"][i1].any()
        assert not c["kf2s"][p]["has_mp"][m12[p][i1]].any()


def test_sft_kitti_two_pairs(oracle_mod, scale):
    c, (nm, m12, F), rs = _sft(oracle_mod, scale, "kitti")
    assert len(c["kf2s"]) == 2 and max(len(k["kps"]) for k in [c["kf1"]] + c["kf2s"]) <= 2000
    assert (nm > 30).all(), nm
    for p, r in enumerate(rs):
        assert np.array_equal(m12[p], r["match12"])
    ex, ey = RP.epipole(c["kf1"]["Tcw"], c["kf2s"][0]["Tcw"])
    assert 0 < ex < RP.W and 0 < ey < RP.H  # forward motion: the epipole is in the image
    assert sum(r["epipole_rejected"] for r in rs) >= 1


@pytest.mark.parametrize("name", ["th_low_edge", "epipole"])
def test_sft_edges(oracle_mod, scale, name):
    c, (nm, m12, F), rs = _sft(oracle_mod, scale, name)
    t = c["tags"]
    assert len(t["match"]) >= 6 and len(t["none"]) >= 4
    for i1, i2 in t["match"]:
        assert m12[0][i1] == i2, (i1, i2, m12[0][i1])
    for i1, i2 in t["none"]:
        assert m12[0][i1] == -1, (i1, i2, m12[0][i1])
    d = [hamming(c["kf1"]["desc"][i1], c["kf2s"][0]["desc"][i2]) for i1, i2 in t["match"] + t["none"]]
    if name == "th_low_edge":
        assert d.count(50) == 3 and d.count(51) == 3
        assert all(hamming(c["kf1"]["desc"][i1], c["kf2s"][0]["desc"][i2]) != 51 for i1, i2 in t["match"])
    else:
        assert rs[0]["epipole_rejected"] == 4  # the mono / mono candidates inside the radius


def test_sft_ties_fall_to_the_later_feature(oracle_mod, scale):
    c, (nm, m12, F), rs = _sft(oracle_mod, scale, "ties")
    node, start, feat = c["kf2s"][0]["fv"]
    for i1, i2 in c["tags"]["winner"]:
        assert m12[0][i1] == i2, (i1, i2, m12[0][i1])
    # the first pair: identical descriptors, both on the line, and the winner is listed later
    i1, i2 = c["tags"]["winner"][0]
    lst = feat.tolist()
    other = [j for j in lst if j != i2 and hamming(c["kf2s"][0]["desc"][j], c["kf1"]["desc"][i1]) == 0]
    assert len(other) == 1 and lst.index(other[0]) < lst.index(i2)


def test_sft_den_zero_and_node_layouts(oracle_mod, scale):
    c, (nm, m12, F), rs = _sft(oracle_mod, scale, "den_zero")
    assert not F.any() and nm[0] == 0 and (m12 == -1).all() and rs[0]["nq"] > 50
    c, (nm, m12, F), rs = _sft(oracle_mod, scale, "one_node")
    assert len(c["kf1"]["fv"][0]) == 1 and len(c["kf1"]["kps"]) == 300 and nm[0] > 30
    c, (nm, m12, F), rs = _sft(oracle_mod, scale, "disjoint")
    assert rs[0]["nq"] == 0 and nm[0] == 0 and (m12 == -1).all()
    c, (nm, m12, F), rs = _sft(oracle_mod, scale, "nq_257")
    assert rs[0]["nq"] == 257 and nm[0] > 30
    c, (nm, m12, F), rs = _sft(oracle_mod, scale, "three_pairs")
    assert len(rs) == 3 and (nm > 10).all() and len({len(k["kps"]) for k in c["kf2s"]}) == 3
    for name in ("empty_kf1", "empty_kf2"):
        c, (nm, m12, F), rs = _sft(oracle_mod, scale, name)
        assert nm[0] == 0 and (m12 == -1).all()
