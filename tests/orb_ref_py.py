"""Independent NumPy restatement of the reference ORB extractor -- TEST INFRASTRUCTURE ONLY.

Written from the reference's src/ORBextractor.cc (ctor :410-470, DivideNode :481-537,
DistributeOctTree :539-763, ComputeKeyPointsOctTree :765-853, IC_Angle :77-104,
computeOrbDescriptor :107-147, operator() :1046-1109, ComputePyramid :1111-1136) and from
SURVEY.md Appendix A items 1-7 for the OpenCV primitives it calls.  It is NOT a translation of
oracle/orb_ref.cpp or of csrc/mmt_orb.hip: its purpose is to be a second reading of the same
sources, so that a misreading shared by the C++ oracle and the kernels does not pass unseen
(tests/test_orb_ref_py.py pins the oracle to it, tests/test_gpu_orb_stages.py the kernels).

Style: integer arithmetic where OpenCV's is integer; np.float32 operations one at a time (NumPy
evaluates every elementwise operation into a rounded float32 temporary, so there is no fused
multiply-add) where the reference computes in float; vectorised over pixels and keys.  Plain
Python loops only in the octree.  Every stage is a function of its own.

Pinned build-dependent choices are SURVEY.md Appendix C's: scalar fixed-point resize (A.4),
error-diffused Q8 Gaussian taps (A.6), portable FAST (A.5), and the octree's sort of (size,
pointer) pairs ordered by (size, node creation sequence) -- DESIGN.md section 2, "Pinned choices".
"""
import math
import os
import re

import numpy as np

F = np.float32

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

PATCH_SIZE = 31       # ORBextractor.cc:72
HALF_PATCH_SIZE = 15  # :73
EDGE_THRESHOLD = 19   # :74
MIN_BORDER = EDGE_THRESHOLD - 3  # :773

_PATTERN_INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "multimot_track_amd", "csrc", "orb_pattern.inc")


def cv_round(v):
    """cvRound: round half to even (Appendix A.2)."""
    return int(np.rint(v))


def load_pattern(path=_PATTERN_INC):
    """bit_pattern_31_ as 512 points (x, y): test q compares points 2q and 2q + 1."""
    ints = []
    for line in open(path):
        line = line.split("//")[0]
        ints += [int(t) for t in re.findall(r"-?\d+", line)]
    assert len(ints) == 1024, len(ints)
    return np.array(ints, np.int32).reshape(512, 2)


# ------------------------------------------------------------------ ctor (:410-470)
def config(nfeatures=2000, scale_factor=1.2, nlevels=8):
    sf = float(F(scale_factor))  # the float argument, stored in a double member (ORBextractor.h:98)
    scale = [F(1.0)]
    for _ in range(1, nlevels):
        scale.append(F(float(scale[-1]) * sf))  # :421 float * double -> float
    inv_scale = [F(1.0) / s for s in scale]     # :429
    factor = F(1.0 / sf)                        # :436
    nd = F(nfeatures) * (F(1) - factor) / (F(1) - F(math.pow(float(factor), float(nlevels))))
    n_per_level, total = [], 0
    for _ in range(nlevels - 1):
        n_per_level.append(cv_round(nd))        # :442
        total += n_per_level[-1]
        nd = nd * factor
    n_per_level.append(max(nfeatures - total, 0))
    # umax (:454-469)
    umax = [0] * (HALF_PATCH_SIZE + 1)
    half = F(HALF_PATCH_SIZE) * np.sqrt(F(2.0)) / F(2)
    vmax = int(math.floor(half + F(1)))
    vmin = int(math.ceil(half))
    for v in range(vmax + 1):
        umax[v] = cv_round(math.sqrt(float(HALF_PATCH_SIZE * HALF_PATCH_SIZE) - v * v))
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return dict(nfeatures=nfeatures, nlevels=nlevels, scale=scale, inv_scale=inv_scale,
                n_per_level=n_per_level, umax=umax)


def level_sizes(w, h, cfg=None):
    """ComputePyramid :1115-1116: cvRound((float)cols * invScale)."""
    cfg = cfg or config()
    return [(cv_round(F(w) * s), cv_round(F(h) * s)) for s in cfg["inv_scale"]]


# ------------------------------------------------------------------ resize (Appendix A.4)
def _resize_coeffs(dn, sn):
    scale = 1.0 / (float(dn) / float(sn))  # cv::resize: inv_scale = (double)dst/src, scale = 1/inv
    d = np.arange(dn, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(F)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(F)
    return s, f


def _sat_short(v):
    return np.clip(np.rint(v).astype(np.int64), -32768, 32767)


def resize_level(src, dw, dh):
    """cv::resize(src, dst, Size(dw, dh), 0, 0, INTER_LINEAR) on 8U, scalar fixed-point path."""
    sh, sw = src.shape
    S = src.astype(np.int64)
    sx, fx = _resize_coeffs(dw, sw)
    lo = sx < 0
    fx = np.where(lo, F(0), fx)
    sx = np.where(lo, 0, sx)
    hi = sx >= sw - 1
    fx = np.where(hi, F(0), fx)
    sx = np.where(hi, sw - 1, sx)
    a0 = _sat_short((F(1) - fx) * F(2048))
    a1 = _sat_short(fx * F(2048))
    sx1 = np.minimum(sx + 1, sw - 1)  # weight a1 is 0 where this clamps
    H = S[:, sx] * a0[None, :] + S[:, sx1] * a1[None, :]
    sy, fy = _resize_coeffs(dh, sh)
    b0 = _sat_short((F(1) - fy) * F(2048))
    b1 = _sat_short(fy * F(2048))
    y0 = np.clip(sy, 0, sh - 1)
    y1 = np.clip(sy + 1, 0, sh - 1)
    v = (b0[:, None] * H[y0] + b1[:, None] * H[y1] + (1 << 21)) >> 22
    return np.clip(v, 0, 255).astype(np.uint8)


def pyramid(gray, cfg=None):
    cfg = cfg or config()
    h, w = gray.shape
    out = [np.ascontiguousarray(gray, np.uint8)]
    for lw, lh in level_sizes(w, h, cfg)[1:]:
        out.append(resize_level(out[-1], lw, lh))
    return out


# ------------------------------------------------------------------ GaussianBlur (Appendix A.6)
GAUSS_TAPS = (18, 34, 48, 56, 48, 34, 18)


def blur7(img):
    """GaussianBlur 7x7 sigma 2, 8U, BORDER_REFLECT_101: Q8 horizontally, Q16 vertically."""
    h, w = img.shape
    p = np.pad(img.astype(np.int64), ((0, 0), (3, 3)), mode="reflect")
    hs = sum(GAUSS_TAPS[k] * p[:, k:k + w] for k in range(7))
    p = np.pad(hs, ((3, 3), (0, 0)), mode="reflect")
    v = sum(GAUSS_TAPS[k] * p[k:k + h] for k in range(7))
    return np.minimum((v + 32768) >> 16, 255).astype(np.uint8)


# ------------------------------------------------------------------ FAST-9/16 (Appendix A.5)
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3),
          (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))


def fast_score_map(img, th):
    """cornerScore<16> (stored as uchar) of every pixel whose circle lies inside img and that
    passes the 9-arc test at threshold th; 0 elsewhere.  A pixel's test and score depend only on
    its 7x7 neighbourhood, so the map of a whole level serves every cell cut from it."""
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return out
    th = min(max(int(th), 0), 255)
    I = img.astype(np.int32)
    v = I[3:h - 3, 3:w - 3]
    d = np.empty((25,) + v.shape, np.int32)
    for k, (dx, dy) in enumerate(CIRCLE):
        d[k] = v - I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx]
    d[16:] = d[:9]

    def arc9(m):  # 9 contiguous circle pixels, circularly
        r = m[0:17].copy()
        for s in range(1, 9):
            r &= m[s:s + 17]
        return r.any(0)

    corner = arc9(d > th) | arc9(d < -th)  # all darker than v - t, or all brighter than v + t
    a0 = np.full(v.shape, th, np.int32)
    for k in range(0, 16, 2):
        a = d[k + 1:k + 9].min(0)
        a0 = np.maximum(a0, np.maximum(np.minimum(a, d[k]), np.minimum(a, d[k + 9])))
    b0 = -a0
    for k in range(0, 16, 2):
        b = d[k + 1:k + 9].max(0)
        b0 = np.minimum(b0, np.minimum(np.maximum(b, d[k]), np.maximum(b, d[k + 9])))
    score = (-b0 - 1) & 0xFF
    out[3:h - 3, 3:w - 3] = np.where(corner, score, 0)
    return out


def nms(S):
    """Strictly greater than all 8 neighbours, scores outside S being 0; row-major (x, y, r)."""
    if S.size == 0:
        return np.zeros((0, 3), F)
    P = np.pad(S, 1)
    h, w = S.shape
    keep = S > 0
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if dy == 1 and dx == 1:
                continue
            keep &= S > P[dy:dy + h, dx:dx + w]
    ys, xs = np.nonzero(keep)
    return np.stack([xs, ys, S[ys, xs]], 1).astype(F)


def fast_cell(img, th):
    """cv::FAST(img, keys, th, nonmaxSuppression=true): keys (x, y, response) in img's frame.
    Corners are detected on rows 3..rows-4 and columns 3..cols-4 only."""
    rows, cols = img.shape
    if rows < 7 or cols < 7:
        return np.zeros((0, 3), F)
    k = nms(fast_score_map(img, th)[3:rows - 3, 3:cols - 3])
    k[:, :2] += F(3)
    return k


# ------------------------------------------------------------------ the cell loop (:769-829)
def level_cells(lw, lh):
    """The FAST cells of a lw x lh level: (i, j, r0, r1, c0, c1, wCell, hCell), in loop order."""
    minBX = minBY = MIN_BORDER
    maxBX, maxBY = lw - EDGE_THRESHOLD + 3, lh - EDGE_THRESHOLD + 3
    W = F(30)
    width, height = F(maxBX - minBX), F(maxBY - minBY)
    nCols, nRows = int(width / W), int(height / W)
    wCell = int(math.ceil(width / F(nCols)))
    hCell = int(math.ceil(height / F(nRows)))
    cells = []
    for i in range(nRows):
        iniY = F(minBY + i * hCell)
        maxY = iniY + F(hCell) + F(6)
        if iniY >= F(maxBY - 3):
            continue
        if maxY > F(maxBY):
            maxY = F(maxBY)
        for j in range(nCols):
            iniX = F(minBX + j * wCell)
            maxX = iniX + F(wCell) + F(6)
            if iniX >= F(maxBX - 6):
                continue
            if maxX > F(maxBX):
                maxX = F(maxBX)
            cells.append((i, j, int(iniY), int(maxY), int(iniX), int(maxX), wCell, hCell))
    return cells


def level_candidates_cells(img, ini_th=20, min_th=7):
    """Per cell of level_cells: the keys FAST leaves in it, (x, y, response) relative to the
    level's minBorder corner (ORBextractor.cc:820-825), iniTh first and minTh if that is empty."""
    lh, lw = img.shape
    s_ini = fast_score_map(img, ini_th)
    s_min = None
    out = []
    for (i, j, r0, r1, c0, c1, wCell, hCell) in level_cells(lw, lh):
        if r1 - r0 < 7 or c1 - c0 < 7:
            k = np.zeros((0, 3), F)
        else:
            k = nms(s_ini[r0 + 3:r1 - 3, c0 + 3:c1 - 3])
            if len(k) == 0:
                if s_min is None:
                    s_min = fast_score_map(img, min_th)
                k = nms(s_min[r0 + 3:r1 - 3, c0 + 3:c1 - 3])
            k[:, 0] += F(3) + F(j * wCell)
            k[:, 1] += F(3) + F(i * hCell)
        out.append(k)
    return out


def level_candidates(img, ini_th=20, min_th=7):
    cells = level_candidates_cells(img, ini_th, min_th)
    return np.concatenate(cells, 0) if cells else np.zeros((0, 3), F)


# ------------------------------------------------------------------ DistributeOctTree (:481-763)
class _Node(object):
    __slots__ = ("ULx", "ULy", "URx", "URy", "BLx", "BLy", "BRx", "BRy", "keys", "no_more",
                 "prev", "next", "seq")

    def __init__(self):
        self.keys = np.zeros(0, np.int64)
        self.no_more = False
        self.prev = self.next = None
        self.seq = -1


class _List(object):
    """std::list: push_front, push_back, erase (returns the successor), front-to-back walk."""

    def __init__(self):
        self.end = _Node()  # sentinel == end()
        self.end.prev = self.end.next = self.end
        self.size = 0
        self.created = 0

    def _link(self, n, before):
        n.prev, n.next = before.prev, before
        before.prev.next = n
        before.prev = n
        self.size += 1
        n.seq = self.created  # creation order: the pinned tie-break of the (size, pointer) sort
        self.created += 1

    def push_back(self, n):
        self._link(n, self.end)

    def push_front(self, n):
        self._link(n, self.end.next)

    def begin(self):
        return self.end.next

    def erase(self, n):
        n.prev.next, n.next.prev = n.next, n.prev
        self.size -= 1
        return n.next


def _divide(p, x, y):
    halfX = int(math.ceil(F(p.URx - p.ULx) / F(2)))  # :483
    halfY = int(math.ceil(F(p.BRy - p.ULy) / F(2)))
    n1, n2, n3, n4 = _Node(), _Node(), _Node(), _Node()
    n1.ULx, n1.ULy = p.ULx, p.ULy
    n1.URx, n1.URy = p.ULx + halfX, p.ULy
    n1.BLx, n1.BLy = p.ULx, p.ULy + halfY
    n1.BRx, n1.BRy = p.ULx + halfX, p.ULy + halfY
    n2.ULx, n2.ULy = n1.URx, n1.URy
    n2.URx, n2.URy = p.URx, p.URy
    n2.BLx, n2.BLy = n1.BRx, n1.BRy
    n2.BRx, n2.BRy = p.URx, p.ULy + halfY
    n3.ULx, n3.ULy = n1.BLx, n1.BLy
    n3.URx, n3.URy = n1.BRx, n1.BRy
    n3.BLx, n3.BLy = p.BLx, p.BLy
    n3.BRx, n3.BRy = n1.BRx, p.BLy
    n4.ULx, n4.ULy = n3.URx, n3.URy
    n4.URx, n4.URy = n2.BRx, n2.BRy
    n4.BLx, n4.BLy = n3.BRx, n3.BRy
    n4.BRx, n4.BRy = p.BRx, p.BRy
    k = p.keys
    left = x[k] < F(n1.URx)
    top = y[k] < F(n1.BRy)
    n1.keys = k[left & top]
    n3.keys = k[left & ~top]
    n2.keys = k[~left & top]
    n4.keys = k[~left & ~top]
    for n in (n1, n2, n3, n4):
        if len(n.keys) == 1:
            n.no_more = True
    return n1, n2, n3, n4


def n_ini(min_x, max_x, min_y, max_y):
    """:543 -- C round() (half away from zero) of a float quotient."""
    q = F(max_x - min_x) / F(max_y - min_y)
    return int(math.floor(float(q) + 0.5)) if q >= 0 else -int(math.floor(-float(q) + 0.5))


def distribute(cands, min_x, max_x, min_y, max_y, N):
    """DistributeOctTree on candidates (x, y, response) relative to (min_x, min_y): the kept keys
    in the order of the final node list (front to back)."""
    cands = np.asarray(cands, F).reshape(-1, 3)
    x, y, resp = cands[:, 0], cands[:, 1], cands[:, 2]
    nIni = n_ini(min_x, max_x, min_y, max_y)
    hX = F(max_x - min_x) / F(nIni)
    L = _List()
    ini = []
    for i in range(nIni):
        n = _Node()
        n.ULx, n.ULy = int(hX * F(i)), 0
        n.URx, n.URy = int(hX * F(i + 1)), 0
        n.BLx, n.BLy = n.ULx, max_y - min_y
        n.BRx, n.BRy = n.URx, max_y - min_y
        L.push_back(n)
        ini.append(n)
    if len(cands):
        which = (x / hX).astype(np.int64)  # :569 float quotient truncated to an index
        for i, n in enumerate(ini):
            n.keys = np.nonzero(which == i)[0]
        assert which.min() >= 0 and which.max() < nIni
    it = L.begin()
    while it is not L.end:
        if len(it.keys) == 1:
            it.no_more = True
            it = it.next
        elif len(it.keys) == 0:
            it = L.erase(it)
        else:
            it = it.next

    def add_children(children, track):
        n_expand = 0
        for c in children:
            if len(c.keys) > 0:
                L.push_front(c)
                if len(c.keys) > 1:
                    n_expand += 1
                    track.append(c)
        return n_expand

    finish = False
    track = []
    while not finish:
        prev_size = L.size
        it = L.begin()
        n_to_expand = 0
        track = []
        while it is not L.end:
            if it.no_more:
                it = it.next
                continue
            n_to_expand += add_children(_divide(it, x, y), track)
            it = L.erase(it)
        if L.size >= N or L.size == prev_size:
            finish = True
        elif L.size + n_to_expand * 3 > N:
            while not finish:
                prev_size = L.size
                prev_track = sorted(track, key=lambda n: (len(n.keys), n.seq))  # :684, pinned tie
                track = []
                for n in reversed(prev_track):
                    add_children(_divide(n, x, y), track)
                    L.erase(n)
                    if L.size >= N:
                        break
                if L.size >= N or L.size == prev_size:
                    finish = True
    keep = []
    it = L.begin()
    while it is not L.end:
        k = it.keys
        keep.append(k[int(np.argmax(resp[k]))])  # first of the largest responses (:747-757)
        it = it.next
    return cands[np.array(keep, np.int64)] if keep else np.zeros((0, 3), F)


# ------------------------------------------------------------------ fastAtan2 (Appendix A.7)
_RAD = F(180.0 / math.pi)
_P1 = F(0.9997878412794807) * _RAD
_P3 = F(-0.3258083974640975) * _RAD
_P5 = F(0.1555786518463281) * _RAD
_P7 = F(-0.04432655554792128) * _RAD
_EPS = F(2.2204460492503131e-16)  # (float)DBL_EPSILON


def fast_atan2(y, x):
    """cv::fastAtan2 in degrees, float32 throughout, vectorised."""
    y = np.asarray(y, F)
    x = np.asarray(x, F)
    ax, ay = np.abs(x), np.abs(y)
    flat = ax >= ay
    num = np.where(flat, ay, ax)
    den = np.where(flat, ax, ay) + _EPS
    with np.errstate(all="ignore"):
        c = num / den
        c2 = c * c
        a = (((_P7 * c2 + _P5) * c2 + _P3) * c2 + _P1) * c
    a = np.where(flat, a, F(90) - a)
    a = np.where(x < 0, F(180) - a, a)
    a = np.where(y < 0, F(360) - a, a)
    return a.astype(F)


def _disc(umax):
    du, dv = [], []
    for v in range(-HALF_PATCH_SIZE, HALF_PATCH_SIZE + 1):
        d = HALF_PATCH_SIZE if v == 0 else umax[abs(v)]
        for u in range(-d, d + 1):
            du.append(u)
            dv.append(v)
    return np.array(du, np.int64), np.array(dv, np.int64)


def ic_moments(img, xs, ys, umax):
    """(m_01, m_10) of IC_Angle (:77-104) for keys at level coordinates (xs, ys), as ints."""
    du, dv = _disc(umax)
    cx = np.rint(np.asarray(xs, F)).astype(np.int64)
    cy = np.rint(np.asarray(ys, F)).astype(np.int64)
    patch = img[cy[:, None] + dv[None, :], cx[:, None] + du[None, :]].astype(np.int64)
    return (patch * dv).sum(1), (patch * du).sum(1)


def ic_angle(img, xs, ys, umax):
    m01, m10 = ic_moments(img, xs, ys, umax)
    return fast_atan2(m01.astype(F), m10.astype(F))


# ------------------------------------------------------------------ computeOrbDescriptor (:107-147)
def descriptors(blurred, xs, ys, angles, pattern):
    n = len(xs)
    if n == 0:
        return np.zeros((0, 32), np.uint8)
    factorPI = F(math.pi / float(F(180)))
    ang = np.asarray(angles, F) * factorPI
    a = np.array([math.cos(float(t)) for t in ang]).astype(F)[:, None]  # (float)cos(angle): libm
    b = np.array([math.sin(float(t)) for t in ang]).astype(F)[:, None]
    px = pattern[:, 0].astype(F)[None, :]
    py = pattern[:, 1].astype(F)[None, :]
    ry = np.rint(px * b + py * a).astype(np.int64)
    rx = np.rint(px * a - py * b).astype(np.int64)
    cx = np.rint(np.asarray(xs, F)).astype(np.int64)[:, None]
    cy = np.rint(np.asarray(ys, F)).astype(np.int64)[:, None]
    v = blurred[cy + ry, cx + rx].astype(np.int32)
    bits = v[:, 0::2] < v[:, 1::2]  # test q = byte q // 8, bit q % 8
    return np.packbits(bits, axis=1, bitorder="little")


# ------------------------------------------------------------------ operator() (:1046-1109)
def orb_stages(gray, nfeatures=2000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7,
               pattern=None):
    """Every stage's result: pyramid, blur (every level), cells (per level, per cell candidate
    arrays), cands, selected (level coordinates, list order), kps, desc."""
    cfg = config(nfeatures, scale_factor, nlevels)
    pattern = load_pattern() if pattern is None else pattern
    pyr = pyramid(np.ascontiguousarray(gray, np.uint8), cfg)
    st = dict(cfg=cfg, pyramid=pyr, blur=[blur7(p) for p in pyr], cells=[], cands=[],
              selected=[])
    kps_all, desc_all = [], []
    for l, img in enumerate(pyr):
        lh, lw = img.shape
        cells = level_candidates_cells(img, ini_th, min_th)
        cands = np.concatenate(cells, 0) if cells else np.zeros((0, 3), F)
        sel = distribute(cands, MIN_BORDER, lw - EDGE_THRESHOLD + 3, MIN_BORDER,
                         lh - EDGE_THRESHOLD + 3, cfg["n_per_level"][l]).copy()
        sel[:, 0] += F(MIN_BORDER)  # :843-844
        sel[:, 1] += F(MIN_BORDER)
        st["cells"].append(cells)
        st["cands"].append(cands)
        st["selected"].append(sel)
        k = np.zeros(len(sel), KP_DTYPE)
        k["x"], k["y"], k["response"] = sel[:, 0], sel[:, 1], sel[:, 2]
        k["octave"] = l
        k["class_id"] = -1
        k["size"] = F(int(F(PATCH_SIZE) * cfg["scale"][l]))  # :837 int scaledPatchSize
        k["angle"] = ic_angle(img, sel[:, 0], sel[:, 1], cfg["umax"]) if len(sel) else 0
        if len(sel) == 0:
            continue
        desc_all.append(descriptors(st["blur"][l], k["x"], k["y"], k["angle"], pattern))
        if l != 0:
            k["x"] = k["x"] * cfg["scale"][l]  # :1099-1105
            k["y"] = k["y"] * cfg["scale"][l]
        kps_all.append(k)
    st["kps"] = np.concatenate(kps_all) if kps_all else np.zeros(0, KP_DTYPE)
    st["desc"] = np.concatenate(desc_all, 0) if desc_all else np.zeros((0, 32), np.uint8)
    return st


def orb_extract(gray, nfeatures=2000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7):
    st = orb_stages(gray, nfeatures, scale_factor, nlevels, ini_th, min_th)
    return st["kps"], st["desc"]


# ------------------------------------------------------------------ comparison helpers
# Shared by tests/test_orb_ref_py.py and tests/test_gpu_orb_stages.py.  All comparisons are exact;
# every helper raises AssertionError naming the stage (tag) and the first differences.
def check_images(tag, got, ref):
    assert len(got) == len(ref), "%s: %d levels against %d" % (tag, len(got), len(ref))
    for l, (a, b) in enumerate(zip(got, ref)):
        assert a.shape == b.shape, "%s: level %d is %s against %s" % (tag, l, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert len(bad) == 0, "%s: level %d differs in %d px, first (y, x) = %s" % (
            tag, l, len(bad), bad[0].tolist())


def check_key_list(tag, got, ref):
    """(n, 3) arrays of (x, y, response): same keys in the same order."""
    got = np.asarray(got, F).reshape(-1, 3)
    ref = np.asarray(ref, F).reshape(-1, 3)
    assert len(got) == len(ref), "%s: %d keys against %d" % (tag, len(got), len(ref))
    bad = np.nonzero((got != ref).any(1))[0]
    assert len(bad) == 0, "%s: %d keys differ, first #%d: %s against %s" % (
        tag, len(bad), bad[0], got[bad[0]].tolist(), ref[bad[0]].tolist())


def check_key_set(tag, got, ref):
    """Same keys (x, y, response) as sets, each once."""
    g = sorted(tuple(int(v) for v in r) for r in np.asarray(got).reshape(-1, 3).tolist())
    r = sorted(tuple(int(v) for v in r) for r in np.asarray(ref).reshape(-1, 3).tolist())
    assert len(set(g)) == len(g), "%s: a key occurs twice" % tag
    only_g = sorted(set(g) - set(r))
    only_r = sorted(set(r) - set(g))
    assert not only_g and not only_r and len(g) == len(r), (
        "%s: %d keys against %d; only here %s, only in the reference %s" %
        (tag, len(g), len(r), only_g[:4], only_r[:4]))


def check_records(tag, k, d, kr, dr):
    """Keypoint records compared as bytes, descriptors equal."""
    assert len(k) == len(kr), "%s: %d keypoints against %d; per level %s against %s" % (
        tag, len(k), len(kr), np.bincount(k["octave"], minlength=8).tolist(),
        np.bincount(kr["octave"], minlength=8).tolist())
    assert k.dtype == KP_DTYPE and kr.dtype == KP_DTYPE
    kb = np.ascontiguousarray(k).view(np.uint8).reshape(len(k), KP_DTYPE.itemsize)
    krb = np.ascontiguousarray(kr).view(np.uint8).reshape(len(kr), KP_DTYPE.itemsize)
    rows = np.nonzero((kb != krb).any(1))[0]
    assert len(rows) == 0, "%s: %d keypoint records differ, first #%d: %s against %s" % (
        tag, len(rows), rows[0], k[rows[0]], kr[rows[0]])
    assert d.shape == dr.shape, "%s: descriptor shapes %s against %s" % (tag, d.shape, dr.shape)
    drow = np.nonzero((d != dr).any(1))[0]
    assert len(drow) == 0, "%s: %d descriptors differ (first #%d)" % (tag, len(drow), drow[0])
