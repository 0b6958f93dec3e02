"""Sequential NumPy restatement of the reference's stereo Frame constructor -- TEST INFRASTRUCTURE
ONLY.

Written from the reference's src/Frame.cc: the constructor :79-159 and Frame::ComputeStereoMatches
:849-1038 (this fork's version: maxD = 200, minD = 0, the vDescIndex output), in the reference's
order, one left key after the other.  It is NOT a translation of csrc/mmt_stereo.hip: the kernels
are pinned to it (tests/test_gpu_stereo.py), and tests/test_stereo_ref_py.py pins it to answers
worked by hand.  Pyramids and keys come from tests/orb_ref_py.py (orb_stages gives pyramid, kps,
desc and cfg).

Style as orb_ref_py: np.float32 operations one at a time where the reference computes in float,
Python ints where it computes in int.

Where the reference is undefined ("Stereo pins"):
  (a) an empty accepted list reads vDistIdx[0] of an empty vector: nothing is cleared, the median
      is reported as -1 and thDist as 0;
  (b) a right key with round(uR0 * invScale) - 10 < 0 would make OpenCV throw in colRange: the
      left key is skipped like the border test (:972) and counted with it;
  (c) ValueError (the library: MMT_EINVAL) for a left key whose 11 x 11 window leaves its level,
      a right key whose row range leaves [0, rows), an octave outside the pyramid.
"""
import math

import numpy as np

F = np.float32

TH_HIGH = 100                          # ORBmatcher.cc
TH_LOW = 50
TH_ORB_DIST = (TH_HIGH + TH_LOW) // 2  # Frame.cc:856
MIN_D = F(0)                           # :883
MAX_D = F(200)                         # :884
W = 5                                  # :959
L = 5                                  # :966

COUNTERS = ("n_coarse", "n_window_edge", "n_end_shift", "n_delta", "n_range", "n_clamped",
            "n_accepted", "n_median_removed", "median", "th_dist")

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def c_round(v):
    """C round() on a float: half away from zero (:954-956)."""
    v = float(F(v))
    return F(math.copysign(math.floor(abs(v) + 0.5), v))


def row_range(y, octave, scale):
    """:873-875: the rows minr..maxr (inclusive) a right key is listed in."""
    r = F(1.2) * F(scale[octave])
    return int(math.floor(F(y) - r)), int(math.ceil(F(y) + r))


def row_table(kps_r, scale, n_rows):
    """:862-879 vRowIndices: per image row the right keys, in ascending key order."""
    rows = [[] for _ in range(n_rows)]
    for i in range(len(kps_r)):
        o = int(kps_r["octave"][i])
        if o < 0 or o >= len(scale):
            raise ValueError("right key %d: octave %d outside the pyramid" % (i, o))
        lo, hi = row_range(kps_r["y"][i], o, scale)
        if lo < 0 or hi >= n_rows:
            raise ValueError("right key %d: rows %d..%d leave [0, %d)" % (i, lo, hi, n_rows))
        for y in range(lo, hi + 1):
            rows[y].append(i)
    return rows


def hamming(a, b):
    """ORBmatcher::DescriptorDistance: set bits of a ^ b over the 32 bytes."""
    return int(_POP[np.bitwise_xor(a, b)].sum())


def parabola(d1, d2, d3):
    """:999 deltaR in float (x / 0 and 0 / 0 as IEEE gives them)."""
    d1, d2, d3 = F(d1), F(d2), F(d3)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (d1 - d3) / (F(2.0) * (d1 + d3 - F(2.0) * d2))


def accept(uL, scale_o, scaled_uR0, best_inc, delta, bf):
    """:1001-1018 from deltaR on: (stage, uR, depth, clamped) with stage one of "delta", "range",
    "ok"."""
    delta = F(delta)
    if delta < F(-1) or delta > F(1):  # a NaN passes
        return "delta", F(-1), F(-1), False
    best_uR = F(scale_o) * (F(scaled_uR0) + F(best_inc) + delta)
    uL = F(uL)
    disparity = uL - best_uR
    if not (disparity >= MIN_D and disparity < MAX_D):
        return "range", F(-1), F(-1), False
    clamped = False
    if disparity <= F(0):
        disparity = F(0.01)                 # :1013 a double literal narrowed to float
        best_uR = F(float(uL) - 0.01)       # :1014 float - double, narrowed
        clamped = True
    return "ok", best_uR, F(bf) / disparity, clamped


def median_threshold(dists):
    """:1023-1025 on the accepted SADs: (median, thDist); (-1, 0) for none (pin a)."""
    if len(dists) == 0:
        return -1, F(0)
    s = sorted(int(d) for d in dists)
    median = s[len(s) // 2]
    return median, F(1.5) * F(1.4) * F(median)


def median_clear_sorted(pairs):
    """:1023-1037 literally: sort the (dist, iL) pairs, walk down from the end, stop at the first
    dist < thDist.  Returns the cleared iL."""
    if not pairs:
        return []
    v = sorted(pairs)
    median = F(v[len(v) // 2][0])
    th = F(1.5) * F(1.4) * median
    out = []
    for i in range(len(v) - 1, -1, -1):
        if F(v[i][0]) < th:
            break
        out.append(v[i][1])
    return out


def median_clear_threshold(pairs):
    """The same as one pass: every accepted key whose (float)dist >= thDist."""
    _, th = median_threshold([p[0] for p in pairs])
    if not pairs:
        return []
    return [i for d, i in pairs if F(d) >= th]


def window(img, u, v):
    """:960-962 / :977-979: the 11 x 11 window around column u, row v as float, minus its centre."""
    w = img[v - W:v + W + 1, u - W:u + W + 1].astype(F)
    return w - w[W, W]


def stereo_matches(pyr_l, pyr_r, kps_l, desc_l, kps_r, desc_r, scale, inv_scale, bf):
    """Frame::ComputeStereoMatches.  Returns dict(uR, depth, right_idx, best_dist, sad, counters):
    best_dist is the coarse search's bestDist (-1 where the search is not reached: an empty row,
    :901 / :907), sad the window search's (-1 where it is not reached)."""
    n = len(kps_l)
    n_rows = pyr_l[0].shape[0]
    nlev = len(pyr_l)
    uR = np.full(n, -1, F)
    depth = np.full(n, -1, F)
    right_idx = np.full(n, -1, np.int32)
    best_dist_out = np.full(n, -1, np.int32)
    sad_out = np.full(n, -1, np.int32)
    C = dict.fromkeys(COUNTERS, 0)
    rows = row_table(kps_r, scale, n_rows)
    # pin (c): every left key's window lies inside its level
    for i in range(n):
        o = int(kps_l["octave"][i])
        if o < 0 or o >= nlev:
            raise ValueError("left key %d: octave %d outside the pyramid" % (i, o))
        s = F(inv_scale[o])
        u, v = int(c_round(F(kps_l["x"][i]) * s)), int(c_round(F(kps_l["y"][i]) * s))
        lh, lw = pyr_l[o].shape
        if u - W < 0 or u + W >= lw or v - W < 0 or v + W >= lh or int(kps_l["y"][i]) >= n_rows:
            raise ValueError("left key %d: its window leaves level %d" % (i, o))
    oct_r = kps_r["octave"].astype(np.int64)
    x_r = kps_r["x"].astype(F)
    pairs = []
    for iL in range(n):
        level = int(kps_l["octave"][iL])
        vL, uL = F(kps_l["y"][iL]), F(kps_l["x"][iL])
        cands = rows[int(vL)]
        if not cands:
            continue
        min_u, max_u = uL - MAX_D, uL - MIN_D
        if max_u < 0:
            continue
        best, best_r = TH_HIGH, 0
        for iR in cands:
            if oct_r[iR] < level - 1 or oct_r[iR] > level + 1:
                continue
            if x_r[iR] >= min_u and x_r[iR] <= max_u:
                d = hamming(desc_l[iL], desc_r[iR])
                if d < best:
                    best, best_r = d, iR
        best_dist_out[iL] = best
        if best_r != 0:            # :943 the quirk: right key 0 is never reported
            right_idx[iL] = best_r
        if best >= TH_ORB_DIST:
            continue
        C["n_coarse"] += 1
        s = F(inv_scale[level])
        su_l = int(c_round(uL * s))
        sv_l = int(c_round(vL * s))
        su_r0 = int(c_round(x_r[best_r] * s))
        img_r = pyr_r[level]
        if su_r0 < 0 or su_r0 + L + W + 1 >= img_r.shape[1] or su_r0 - L - W < 0:  # :972, pin (b)
            C["n_window_edge"] += 1
            continue
        il = window(pyr_l[level], su_l, sv_l)
        best_sad, best_inc = 2 ** 31 - 1, 0
        dists = [F(0)] * (2 * L + 1)
        for inc in range(-L, L + 1):
            ir = window(img_r, su_r0 + inc, sv_l)
            dist = F(np.abs(il - ir).astype(np.float64).sum())  # cv::norm: a double, to float
            if dist < F(best_sad):
                best_sad, best_inc = int(dist), inc
            dists[L + inc] = dist
        sad_out[iL] = best_sad
        if best_inc == -L or best_inc == L:
            C["n_end_shift"] += 1
            continue
        delta = parabola(dists[L + best_inc - 1], dists[L + best_inc], dists[L + best_inc + 1])
        stage, u, z, clamped = accept(uL, scale[level], su_r0, best_inc, delta, bf)
        if stage == "delta":
            C["n_delta"] += 1
        elif stage == "range":
            C["n_range"] += 1
        else:
            C["n_clamped"] += int(clamped)
            C["n_accepted"] += 1
            uR[iL], depth[iL] = u, z
            pairs.append((best_sad, iL))
    C["median"], C["th_dist"] = median_threshold([p[0] for p in pairs])
    for iL in median_clear_sorted(pairs):
        uR[iL] = depth[iL] = -1
        right_idx[iL] = -1
        C["n_median_removed"] += 1
    return dict(uR=uR, depth=depth, right_idx=right_idx, best_dist=best_dist_out, sad=sad_out,
                counters=C)


def stereo_frame(left, right, mask=None, nfeatures=2000, bf=387.5744):
    """The stereo Frame constructor (:79-159): both sides extracted, vSemLabel, the matches."""
    import orb_ref_py as R
    sl = R.orb_stages(left, nfeatures)
    sr = R.orb_stages(right, nfeatures)
    cfg = sl["cfg"]
    out = dict(kps=sl["kps"], desc=sl["desc"], kps_right=sr["kps"], desc_right=sr["desc"])
    n = len(sl["kps"])
    if n == 0:  # :103 the early return
        out.update(uR=np.zeros(0, F), depth=np.zeros(0, F), right_idx=np.zeros(0, np.int32),
                   sem_label=np.zeros(0, np.int32), counters=dict.fromkeys(COUNTERS, 0))
        out["counters"]["median"] = -1
        return out
    if mask is not None:  # :116-124
        out["sem_label"] = mask[sl["kps"]["y"].astype(np.int64),
                                sl["kps"]["x"].astype(np.int64)].astype(np.int32)
    out.update(stereo_matches(sl["pyramid"], sr["pyramid"], sl["kps"], sl["desc"], sr["kps"],
                              sr["desc"], cfg["scale"], cfg["inv_scale"], bf))
    return out
