"""Synthetic keyframes that put a search window on the boundaries of the matchers' shared cell
walk (GetFeaturesInArea's cell range scanned 64 keys per pass): a pile of keys with one
descriptor in two adjacent cells whose cell range holds an exact number of keys, a window of one
cell in the image's last column and row, a window whose cells are empty, and keys with the pile's
descriptor far from it (inside a window that covers the whole image only).  The camera is at the
origin (identity pose), KITTI intrinsics, 8 levels at factor 1.2.  These are inputs, and NumPy
statements of which cells and keys a window reaches for the tests' own preconditions; expected
outputs come from the CPU oracle and tests/sim3_ref_py.py."""
import math

import numpy as np

from orb_ref_py import KP_DTYPE
from sim3_cases import H, K_KITTI, W, orb_scales

f32 = np.float32
COLS, ROWS = 64, 48
INV_W, INV_H = f32(COLS) / f32(W), f32(ROWS) / f32(H)
LEVEL = 2          # the level every point predicts; keys at LEVEL - 1 and LEVEL are compared
WRONG_OCTAVE = 5   # a key no matcher here compares with a point at LEVEL
PILE_COL, PILE_ROW = 20, 20  # the pile straddles columns 19 | 20 of row 20
PILE_UV = (float((PILE_COL - 0.5) / INV_W), float(PILE_ROW / INV_H))
EMPTY_UV = (780.0, 80.0)
CORNER_UV = (1234.0, 372.5)
CORNER_KEYS = ((1231.8, 370.5), (1231.0, 369.5))
TWIN_CELLS = ((2, 30), (30, 30), (62, 30))


def cell_of(x, y):
    """PosInGrid: C round() of the float product; None outside the grid."""
    px = int(math.floor(float(f32(x) * INV_W) + 0.5))
    py = int(math.floor(float(f32(y) * INV_H) + 0.5))
    return (px, py) if 0 <= px < COLS and 0 <= py < ROWS else None


def cell_range(u, v, r):
    """GetFeaturesInArea's cell range (cx0, cx1, cy0, cy1) of a window inside the image."""
    u, v, r = f32(u), f32(v), f32(r)
    return (max(0, int(math.floor(f32(u - r) * INV_W))),
            min(COLS - 1, int(math.ceil(f32(u + r) * INV_W))),
            max(0, int(math.floor(f32(v - r) * INV_H))),
            min(ROWS - 1, int(math.ceil(f32(v + r) * INV_H))))


def keys_in_range(cell_start, cell_idx, rng4):
    """The keys of a cell range in GetFeaturesInArea order, from the CSR grid (cells ix*48+iy)."""
    cx0, cx1, cy0, cy1 = rng4
    out = []
    for ix in range(cx0, cx1 + 1):
        out += list(cell_idx[cell_start[ix * ROWS + cy0]:cell_start[ix * ROWS + cy1 + 1]])
    return out


def point_at(u, v, z=10.0, level=LEVEL):
    """A map point that projects to (u, v) and predicts `level`: (Xw, normal, min_dist, max_dist)."""
    fx, fy, cx, cy = K_KITTI
    X = np.array([(u - cx) * z / fx, (v - cy) * z / fy, z])
    d = np.linalg.norm(X)
    maxd = d * 1.2 ** (level - 0.5)
    return X.astype(f32), (X / d).astype(f32), f32(maxd / 1.2 ** 7), f32(maxd)


def walk_keyframe(n_pile, winner, n_background=60, seed=5):
    """A keyframe of n_pile + 5 + n_background keys and its three map points (pile, empty, corner).

    The pile's keys alternate between the two cells, the even ones in the later column, so the
    first key in GetFeaturesInArea order is not the lowest index.  winner "first": every pile key
    is at LEVEL; "last": only the last one in that order is, the others at WRONG_OCTAVE.
    Returns dict(kps, desc, depth, D, points=dict(Xw, normal, min_dist, max_dist, pdesc))."""
    rng = np.random.default_rng(seed)
    D = rng.integers(0, 256, 32, dtype=np.uint8)
    xy, octs, descs = [], [], []
    for i in range(n_pile):
        later = i % 2 == 0
        xy.append((PILE_UV[0] + (1.0 if later else -1.0), PILE_UV[1] + 0.2 * ((i // 2) % 5 - 2)))
        octs.append(LEVEL if winner == "first" else WRONG_OCTAVE)
        descs.append(D)
    if winner == "last":
        octs[n_pile - 1 if (n_pile - 1) % 2 == 0 else n_pile - 2] = LEVEL
    for x, y in CORNER_KEYS:
        xy.append((x, y))
        octs.append(LEVEL)
        descs.append(D)
    for cx, cy in TWIN_CELLS:  # the pile's descriptor far from every window but the whole image
        xy.append((float(cx / INV_W), float(cy / INV_H)))
        octs.append(LEVEL)
        descs.append(D)
    keep_out = [(PILE_COL - 3, PILE_COL + 3, PILE_ROW - 3, PILE_ROW + 4), (60, 63, 43, 47)]
    ec = cell_of(*EMPTY_UV)
    keep_out.append((ec[0] - 3, ec[0] + 3, ec[1] - 3, ec[1] + 3))
    while len(xy) < n_pile + 5 + n_background:
        x, y = float(rng.uniform(5, W - 5)), float(rng.uniform(5, H - 5))
        c = cell_of(x, y)
        if c is None or any(a <= c[0] <= b and lo <= c[1] <= hi for a, b, lo, hi in keep_out):
            continue
        xy.append((x, y))
        octs.append(int(rng.integers(0, 8)))
        descs.append(rng.integers(0, 256, 32, dtype=np.uint8))
    n = len(xy)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"], kps["y"] = np.array(xy, f32).T
    kps["octave"], kps["size"] = octs, 31.0
    pts = [point_at(*PILE_UV), point_at(*EMPTY_UV), point_at(*CORNER_UV)]
    points = dict(Xw=np.stack([p[0] for p in pts]), normal=np.stack([p[1] for p in pts]),
                  min_dist=np.array([p[2] for p in pts], f32),
                  max_dist=np.array([p[3] for p in pts], f32), pdesc=np.stack([D, D, D]))
    return dict(kps=kps, desc=np.stack(descs), depth=np.zeros((H, W), f32), D=D, points=points)


def radius(r0, level=LEVEL):
    """A matcher's window radius at `level`: its radius at level 0 times the scale factor."""
    return f32(r0) * orb_scales()[0][level]


def sim3_pair(kf):
    """walk_keyframe's points as keyframe 1 (one key per point, away from the windows) and its
    keys as keyframe 2 without points, under the identity similarity."""
    P = kf["points"]
    m = len(P["min_dist"])
    k1 = np.zeros(m, KP_DTYPE)
    k1["x"], k1["y"], k1["size"] = 100.0 + 30.0 * np.arange(m), 300.0, 31.0
    n = len(kf["kps"])
    eye = np.eye(4, dtype=f32)
    kf1 = dict(kps=k1, desc=np.zeros((m, 32), np.uint8), depth=kf["depth"], Tcw=eye, Xw=P["Xw"],
               min_dist=P["min_dist"], max_dist=P["max_dist"], pdesc=P["pdesc"],
               skip=np.zeros(m, np.uint8))
    kf2 = dict(kps=kf["kps"], desc=kf["desc"], depth=kf["depth"], Tcw=eye,
               Xw=np.zeros((n, 3), f32), min_dist=np.ones(n, f32), max_dist=np.ones(n, f32),
               pdesc=np.zeros((n, 32), np.uint8), skip=np.ones(n, np.uint8))
    return kf1, kf2, dict(s=f32(1.0), R=np.eye(3, dtype=f32), t=np.zeros(3, f32))


def rescan_case(n_points=10, copies=12, n_keys=13, seed=9):
    """SearchLocalPoints inputs whose later copies of a point find their kCandK = 8 candidates
    taken: n_points points, `copies` of each in a row, each with n_keys keys in its window at
    Hamming distances 0, 4, 6, 8, 11, ... (each at most 0.8 of the next, so every copy's best
    unbound key passes the ratio test against the one after it)."""
    rng = np.random.default_rng(seed)
    dists = [0, 4, 6, 8, 11, 14, 18, 23, 29, 37, 47, 59, 74][:n_keys]
    xy, descs, pts = [], [], []
    for j in range(n_points):
        u, v = 100.0 + 110.0 * j, 60.0 + 25.0 * j
        D = rng.integers(0, 256, 32, dtype=np.uint8)
        bits = np.unpackbits(D)
        order = rng.permutation(256)
        for e in rng.permutation(n_keys):  # distances in no particular key order
            b = bits.copy()
            b[order[:dists[e]]] ^= 1
            xy.append((u + 0.4 * (e % 4) - 0.6, v + 0.4 * (e // 4) - 0.6))
            descs.append(np.packbits(b))
        pts.append(point_at(u, v) + (D,))
    kps = np.zeros(len(xy), KP_DTYPE)
    kps["x"], kps["y"] = np.array(xy, f32).T
    kps["octave"], kps["size"] = LEVEL, 31.0

    def rep(a):
        return np.repeat(np.stack(a), copies, 0)
    return dict(kps=kps, desc=np.stack(descs), depth=np.zeros((H, W), f32),
                Xw=rep([p[0] for p in pts]), normal=rep([p[1] for p in pts]),
                min_dist=rep([p[2] for p in pts]), max_dist=rep([p[3] for p in pts]),
                pdesc=rep([p[4] for p in pts]), n_keys=n_keys, copies=copies)
