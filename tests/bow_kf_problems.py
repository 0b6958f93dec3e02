"""Inputs of ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*): keyframe 1 (replayed) and keyframe 2
(scanned) as (fv, kps, desc, mp_ok) tuples, fv = (node ids ascending, starts, features).
kf_problem wraps bow_problems.bow_problem (its keyframe is keyframe 1, its frame keyframe 2) and
adds the MapPoint flags of side 2; keyframe1 / candidate / sized_problem set every node's size
exactly, for one keyframe 1 and any number of candidates;
hand builds a case of a few keys from descriptors with chosen Hamming distances."""
import numpy as np

import bow_problems as BP


def kf_problem(seed, mp_valid2=0.85, **kw):
    fv1, kps1, desc1, ok1, fv2, kps2, desc2 = BP.bow_problem(seed, **kw)
    rng = np.random.default_rng(seed + 5000)
    ok2 = (rng.uniform(size=len(kps2)) < mp_valid2).astype(np.uint8)
    return (fv1, kps1, desc1, ok1), (fv2, kps2, desc2, ok2)


def flip_bits(rng, desc, nflip):
    d = np.unpackbits(desc)
    d[rng.choice(256, nflip, replace=False)] ^= 1
    return np.packbits(d)


def keyframe1(seed, sizes1, mp_valid=0.85, shuffle=False):
    """Keyframe 1 with sizes1[k] keys in node k (id 3 k + 1; 0: no such node), spread over the key
    indices at random."""
    rng = np.random.default_rng(seed)
    sizes1 = np.asarray(sizes1, np.int64)
    n1 = int(sizes1.sum())
    nodes1 = rng.permutation(np.repeat(3 * np.arange(len(sizes1)) + 1, sizes1))
    desc1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    ok1 = (rng.uniform(size=n1) < mp_valid).astype(np.uint8)
    srng = np.random.default_rng(seed + 1000) if shuffle else None
    return BP.feature_vector(nodes1, srng), BP._kps(rng, n1), desc1, ok1


def node_of_key(kf):
    """The node id of every key of a keyframe (-1: in no node)."""
    (node, start, feat), kps = kf[0], kf[1]
    out = np.full(len(kps), -1, np.int64)
    for k, nid in enumerate(node):
        out[feat[start[k]:start[k + 1]]] = int(nid)
    return out


def candidate(seed, kf1, sizes2, frac_match=0.6, rot=12.0, rot_outliers=0.15, mp_valid=0.85,
              shuffle=False, dup=0.05):
    """A keyframe 2 for keyframe1's kf1 with sizes2[k] keys in node k.  In every node a share of
    its keys are bit-flipped copies (0..69 bits) of distinct keys of keyframe 1 in the same node,
    turned by `rot` degrees with some rotation outliers, and a few more are exact copies of those
    copies (equal distances)."""
    rng = np.random.default_rng(seed)
    _, kps1, desc1, _ = kf1
    nodes1 = node_of_key(kf1)
    sizes2 = np.asarray(sizes2, np.int64)
    ids = 3 * np.arange(len(sizes2)) + 1
    n2 = int(sizes2.sum())
    nodes2 = rng.permutation(np.repeat(ids, sizes2))
    desc2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    kps2 = BP._kps(rng, n2)
    for nid in ids:
        a, b = np.nonzero(nodes1 == nid)[0], np.nonzero(nodes2 == nid)[0]
        m = min(int(frac_match * len(b)), len(a))
        if m == 0:
            continue
        src, perm = rng.permutation(a)[:m], rng.permutation(b)
        dst, rest = perm[:m], perm[m:]
        for s, t in zip(src, dst):
            desc2[t] = flip_bits(rng, desc1[s], int(rng.integers(0, 70)))
            ang = kps1["angle"][s] - rot + rng.normal(0, 2.0)
            if rng.uniform() < rot_outliers:
                ang = rng.uniform(0, 360)
            kps2["angle"][t] = np.float32(ang % 360.0)
        for j in range(min(int(dup * m), len(rest))):
            desc2[rest[j]] = desc2[dst[j]]
            kps2["angle"][rest[j]] = kps2["angle"][dst[j]]
    ok2 = (rng.uniform(size=n2) < mp_valid).astype(np.uint8)
    srng = np.random.default_rng(seed + 1000) if shuffle else None
    return BP.feature_vector(nodes2, srng), kps2, desc2, ok2


def sized_problem(seed, sizes1, sizes2, mp_valid1=0.85, mp_valid2=0.85, shuffle=False, **kw):
    """(keyframe 1, keyframe 2) with every node's size set on both sides."""
    kf1 = keyframe1(seed, sizes1, mp_valid1, shuffle)
    return kf1, candidate(seed + 7, kf1, sizes2, mp_valid=mp_valid2, shuffle=shuffle, **kw)


EMPTY_FV = (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.int32))


def bits(*idx):
    """The descriptor whose set bits are idx (ints or ranges): the Hamming distance of two such
    descriptors is the size of the symmetric difference of their bit sets."""
    d = np.zeros(256, np.uint8)
    for i in idx:
        d[list(i) if isinstance(i, range) else i] = 1
    return np.packbits(d)


def hand(desc, nodes, ok=None, angle=None):
    """A keyframe from a list of descriptors and {node id: [keys in list order]}."""
    n = len(desc)
    kps = np.zeros(n, BP.KP_DTYPE)
    if angle is not None:
        kps["angle"] = np.asarray(angle, np.float32)
    ids = sorted(nodes)
    start, feat = [0], []
    for i in ids:
        feat.extend(nodes[i])
        start.append(len(feat))
    fv = (np.asarray(ids, np.uint32), np.asarray(start, np.int32), np.asarray(feat, np.int32))
    ok = np.ones(n, np.uint8) if ok is None else np.asarray(ok, np.uint8)
    return fv, kps, np.asarray(desc, np.uint8).reshape(n, 32), ok


def case_49_50():
    """Two nodes of one pair each: distance 49 and distance 50.  Expected match12 = [0, -1]."""
    kf1 = hand([bits(), bits()], {4: [0], 8: [1]})
    kf2 = hand([bits(range(49)), bits(range(50))], {4: [0], 8: [1]})
    return kf1, kf2


def case_no_mappoint():
    """One key of keyframe 1 at distances 10, 30, 35 from keys 0, 1, 2 of keyframe 2; keys 0 and 2
    hold no MapPoint.  Expected match12 = [1] with (bestDist1, bestDist2) = (30, 256): counted,
    key 0 would win and key 2 would fail the ratio test (30 < 0.75 * 35 is false)."""
    kf1 = hand([bits()], {2: [0]})
    kf2 = hand([bits(range(10)), bits(range(30)), bits(range(35))], {2: [0, 1, 2]}, ok=[0, 1, 0])
    return kf1, kf2
