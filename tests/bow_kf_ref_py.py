"""Sequential restatement of ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&)
(ORBmatcher.cc:897-1030) in Python, written from the reference's text: the lower_bound walk over
the two FeatureVectors, the double loop with its running (bestDist1, bestDist2), the strict TH_LOW
threshold, the ratio test in float, the rotation histogram of keyframe-1 keys and
ComputeThreeMaxima (ORBmatcher.cc:2233-2275).  A keyframe is (fv, kps, desc, mp_ok) with fv =
(node ids ascending, starts, features).  Returns (nmatches, match12, trace): match12[i1] = the key
of keyframe 2 whose MapPoint vpMatches12[i1] holds, or -1; trace[i1] = (bestDist1, bestDist2,
bestIdx2) of every replayed feature of keyframe 1, before the threshold."""
import bisect

import numpy as np

TH_LOW = 50
HISTO_LENGTH = 30

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def descriptor_distance(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def c_round(x):
    """C round() of a float: half away from zero."""
    x = float(x)
    return int(np.floor(x + 0.5)) if x >= 0 else -int(np.floor(-x + 0.5))


def compute_three_maxima(sizes):
    """ComputeThreeMaxima over the bins' sizes -> (ind1, ind2, ind3)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3 = s
            ind3 = i
    if np.float32(max2) < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif np.float32(max3) < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def scan_loop(dist, idx2):
    """The inner loop of ORBmatcher.cc:950-976 over the distances of the keys it does not skip."""
    best1, best2, best_idx2 = 256, 256, -1
    for d, i2 in zip(dist.tolist(), idx2.tolist()):
        if d < best1:
            best2 = best1
            best1 = d
            best_idx2 = i2
        elif d < best2:
            best2 = d
    return best1, best2, best_idx2


def scan_fast(dist, idx2):
    """What scan_loop leaves, without the loop (a node of 16384 keys): the smallest distance, the
    first key in list order that has it, and the second smallest of all distances counting ties
    (an equal distance fails '<' and falls to the 'else if').  test_bow_kf_ref_py pins it to
    scan_loop."""
    if len(dist) == 0:
        return 256, 256, -1
    t = int(np.argmin(dist))  # the first of equal minima
    rest = np.delete(dist, t)
    best2 = min(int(rest.min()), 256) if len(rest) else 256
    return int(dist[t]), best2, int(idx2[t])


def search_by_bow_kf(kf1, kf2, nnratio=0.75, check_orientation=True, literal=False):
    (node1, start1, feat1), kps1, desc1, ok1 = kf1
    (node2, start2, feat2), kps2, desc2, ok2 = kf2
    node1 = [int(x) for x in node1]
    node2 = [int(x) for x in node2]
    n1, n2 = len(kps1), len(kps2)
    match12 = np.full(n1, -1, np.int32)
    matched2 = np.zeros(max(n2, 1), bool)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    factor = np.float32(1.0) / np.float32(HISTO_LENGTH)
    ratio = np.float32(nnratio)
    trace = {}
    nmatches = 0
    # the distances of a node pair at once (the loop below reads them one by one, in order)
    i, j = 0, 0
    while i < len(node1) and j < len(node2):
        if node1[i] == node2[j]:
            f1 = [int(x) for x in feat1[start1[i]:start1[i + 1]]]
            f2 = [int(x) for x in feat2[start2[j]:start2[j + 1]]]
            f2 = np.asarray(f2, np.int64)
            live2 = f2[np.asarray(ok2)[f2] != 0]  # pMP2 != NULL and !isBad()
            for idx1 in f1:
                if not ok1[idx1]:  # pMP1 == NULL or isBad()
                    continue
                # keys of keyframe 2 the inner loop does not skip, in list order
                open2 = live2[~matched2[live2]]
                dist = _POP[np.bitwise_xor(desc2[open2], desc1[idx1][None, :])].sum(axis=1)
                best1, best2, best_idx2 = (scan_loop if literal else scan_fast)(dist, open2)
                trace[idx1] = (best1, best2, best_idx2)
                if best1 < TH_LOW:
                    if np.float32(best1) < ratio * np.float32(best2):
                        match12[idx1] = best_idx2
                        matched2[best_idx2] = True
                        if check_orientation:
                            rot = np.float32(kps1["angle"][idx1]) - np.float32(kps2["angle"][best_idx2])
                            if rot < 0.0:
                                rot = np.float32(rot + np.float32(360.0))
                            b = c_round(np.float32(rot * factor))
                            if b == HISTO_LENGTH:
                                b = 0
                            assert 0 <= b < HISTO_LENGTH
                            rot_hist[b].append(idx1)
                        nmatches += 1
            i += 1
            j += 1
        elif node1[i] < node2[j]:
            i = bisect.bisect_left(node1, node2[j])  # vFeatVec1.lower_bound(f2it->first)
        else:
            j = bisect.bisect_left(node2, node1[i])
    if check_orientation:
        ind = compute_three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b in ind:
                continue
            for idx1 in rot_hist[b]:
                match12[idx1] = -1
                nmatches -= 1
    return nmatches, match12, trace
