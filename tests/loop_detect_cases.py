"""Inputs of the loop-detection tests: hand cases whose outcomes follow by hand (vectors of 2 to 8
words, values exact binary fractions, L1 scoring) and a seeded revisit scenario.

A hand case is a function of `make`, which returns a fresh detector with the methods of
loop_detect_ref_py.RefLoop (set_bow, db_add, db_erase, candidates, detect_loop, groups as a
property or attribute, score): the restatement on the CPU, the library on the GPU.  Every expected
value below is worked out in the comments, not taken from either.
"""
import numpy as np

F = np.float32


def graph(n, ordered=None, conn=None, bad=()):
    g = dict(ordered=[[] for _ in range(n)], conn=[[] for _ in range(n)], bad=[0] * n)
    for k, v in (ordered or {}).items():
        g["ordered"][k] = list(v)
    for k, v in (conn or {}).items():
        g["conn"][k] = list(v)
    for k in bad:
        g["bad"][k] = 1
    return g


def _fill(d, vecs, add):
    for k, (w, v) in vecs.items():
        d.set_bow(k, w, v)
    for k in add:
        d.db_add(k)


def case_identical(make):
    """Two identical vectors: every term is |0| - 2 vi, the sum -2 (exact), the score exactly 1."""
    d = make(0)
    v = ([1, 2, 3], [0.5, 0.25, 0.25])
    _fill(d, {0: v, 1: v}, [0])
    assert d.score(1, 0) == 1.0
    assert d.candidates(1, 1.0, graph(2)) == [0]


ORDER_VECS = {  # the query 4 = {10: .5, 20: .5}; each other shares one word at .5: term -1, score .5
    0: ([20, 21], [0.5, 0.5]), 1: ([10, 11], [0.5, 0.5]), 2: ([20, 22], [0.5, 0.5]),
    3: ([10, 12], [0.5, 0.5]), 4: ([10, 20], [0.5, 0.5])}


def case_order(make):
    """lKFsSharingWords: word 10's list [1, 3] (add order), then word 20's [0, 2].  maxCommonWords 1,
    minCommonWords (int)0.8f = 0: all pass; all score .5 > .75 * .5.  Then erase keeps the others'
    order, and a keyframe added again goes to the end of its words' lists."""
    d = make(0)
    _fill(d, ORDER_VECS, [0, 1, 2, 3])
    g = graph(5)
    assert d.candidates(4, 0.0, g) == [1, 3, 0, 2]
    assert d.candidates(4, 0.0, g) == [1, 3, 0, 2]  # the same query twice
    d.db_erase(1)
    assert d.candidates(4, 0.0, g) == [3, 0, 2]
    d.db_erase(1)  # erase of a non-member does nothing
    assert d.candidates(4, 0.0, g) == [3, 0, 2]
    d.db_add(1)
    assert d.candidates(4, 0.0, g) == [3, 1, 0, 2]


EIGHT = (list(range(1, 9)), [0.125] * 8)


def case_connected(make):
    """Query 2 = eight words at 1/8.  Keyframe 0 is identical but connected: it is left out, and
    its 8 common words do not count (with them minCommonWords would be 6 and keyframe 1, which
    shares 2 words, would fail).  Keyframe 1 = {1: .5, 2: .5}: two terms |1/8 - 1/2| - 5/8 = -1/4,
    score 1/4.  si == minScore passes; the next float32 above it does not."""
    d = make(0)
    _fill(d, {0: EIGHT, 1: ([1, 2], [0.5, 0.5]), 2: EIGHT}, [0, 1])
    g = graph(3, conn={2: [0]})
    assert d.candidates(2, 0.25, g) == [1]
    assert d.candidates(2, np.nextafter(F(0.25), F(1)), g) == []
    assert d.candidates(2, 0.25, graph(3)) == [0]  # unconnected, 0 alone passes the word filter


def case_common_words(make):
    """maxCommonWords 5 -> minCommonWords (int)(5 * 0.8f) = 4: keyframe 1 with 4 common words
    fails, 0 and 2 with 5 pass.  Scores: 0 and 2 are 3 terms of -1/4 and 2 of -1/4 (|0| - 1/4):
    sum -5/4, score 5/8; keyframe 1 would score 1/2 > 3/4 * 5/8 and stay if it were scored."""
    d = make(0)
    five = [0.25, 0.25, 0.25, 0.125, 0.125]
    _fill(d, {0: ([1, 2, 3, 4, 5], five), 1: ([1, 2, 3, 4], [0.25] * 4),
              2: ([4, 5, 6, 7, 8], five[::-1]), 3: EIGHT}, [0, 1, 2])
    assert d.score(3, 0) == 0.625 and d.score(3, 1) == 0.5 and d.score(3, 2) == 0.625
    assert d.candidates(3, 0.0, graph(4)) == [0, 2]


CUT_VECS = {  # the query 2 = {1: 1/2, 2: 1/4, 3: 1/8, 4: 1/8}
    0: ([1, 2, 3, 4], [0.25] * 4),  # terms -1/2, -1/2, -1/4, -1/4: score 3/4
    1: ([1, 2, 3, 4], [0.5, 0.25, 0.125, 0.125]),  # identical: score 1
    2: ([1, 2, 3, 4], [0.5, 0.25, 0.125, 0.125])}


def case_cut(make):
    """bestAccScore 1, minScoreToRetain 0.75f: keyframe 0's accumulated 0.75 is not above it."""
    d = make(0)
    _fill(d, CUT_VECS, [0, 1])
    assert d.score(2, 0) == 0.75 and d.score(2, 1) == 1.0
    assert d.candidates(2, 0.0, graph(3)) == [1]


def case_duplicate(make):
    """Keyframes 0 and 1 list each other as best covisibles: both accumulate 1.75 and both name
    keyframe 1 (score 1 > 3/4; 3/4 > 1 is false) as pBestKF: it is returned once."""
    d = make(0)
    _fill(d, CUT_VECS, [0, 1])
    assert d.candidates(2, 0.0, graph(3, ordered={0: [1], 1: [0]})) == [1]


def _detect_vecs():
    v = {0: ([1, 2], [0.5, 0.5]), 1: ([1, 2, 3, 4], [0.25] * 4), 2: EIGHT}
    v[10] = EIGHT
    return v


def case_min_score(make):
    """DetectLoop for keyframe 10 (eight words at 1/8), mLastLoopKFid 0.  Its covisibles: 0 (bad,
    score 1/4) and 1 (four terms |1/8 - 1/4| - 3/8 = -1/4: score 1/2): minScore is 1/2, not 1/4.
    Keyframe 2 is identical (score 1) and unconnected: the one candidate, in a new group."""
    d = make(0)
    _fill(d, _detect_vecs(), [0, 1, 2])
    g = graph(11, ordered={10: [0, 1]}, conn={10: [0, 1]}, bad=[0])
    r = d.detect_loop(10, 0, g)
    assert r["ran"] and r["min_score"] == F(0.5)
    assert r["candidates"] == [2] and r["enough"] == [] and r["n_groups"] == 1
    assert list(d.groups) == [([2], 0)]


def case_no_covisible(make):
    """No covisible keyframe: minScore stays 1, and only the identical keyframe 2 reaches it."""
    d = make(0)
    _fill(d, _detect_vecs(), [0, 1, 2])
    r = d.detect_loop(10, 0, graph(11))
    assert r["ran"] and r["min_score"] == F(1)
    assert r["candidates"] == [2]


def case_groups(make):
    """Keyframes 10..13 repeat keyframe 0's vector; each is connected (not covisible) to the ones
    before, so keyframe 0 is the one candidate every time.  Its group {0, 1} meets the previous
    group: the counter runs 0, 1, 2, 3, and with the threshold 3 the fourth call reports it.
    Keyframe 9 takes the early exit (9 < 0 + 10) and is only added.  Then keyframe 14 shares no
    word: no candidate, and the groups are cleared."""
    d = make(0)
    v = ([1, 2, 3], [0.5, 0.25, 0.25])
    vecs = {0: v, 9: ([50], [1.0]), 14: ([60], [1.0])}
    for k in range(10, 14):
        vecs[k] = v
    _fill(d, vecs, [0])
    conn = {k: list(range(10, k)) for k in range(10, 14)}
    conn[0] = [1]
    g = graph(15, conn=conn)
    r = d.detect_loop(9, 0, g)
    assert not r["ran"] and r["candidates"] == [] and r["n_groups"] == 0
    for n, k in enumerate(range(10, 14)):
        r = d.detect_loop(k, 0, g)
        assert r["ran"] and r["min_score"] == F(1) and r["candidates"] == [0]
        assert list(d.groups) == [([0, 1], n)]
        assert r["enough"] == ([0] if n >= 3 else [])
    r = d.detect_loop(14, 0, g)
    assert r["ran"] and r["candidates"] == [] and r["n_groups"] == 0 and list(d.groups) == []


HAND_CASES = [case_identical, case_order, case_connected, case_common_words, case_cut,
              case_duplicate, case_min_score, case_no_covisible, case_groups]


# ---- the seeded revisit scenario ---------------------------------------------------------------
def scenario(seed=7, n_kf=120, n_places=60, scoring=0):
    """Two laps round a ring of n_places places, one keyframe per step.  Returns (vectors, steps):
    vectors[k] = (words, values), L1-normalised in word order; steps[k] = dict(graph, erase) = the
    covisibility graph when keyframe k reaches DetectLoop and the keyframes erased (and bad) from
    then on.  Covisibility is between temporal neighbours; weights below the threshold stay out of
    `ordered`, so `conn` is the larger list.  Three keyframes see something no other does (no
    common word: no candidate, which clears the groups)."""
    rng = np.random.default_rng(seed)
    pools = [np.sort(rng.choice(20000, 260, replace=False)) for _ in range(n_places)]
    shared = np.sort(rng.choice(np.arange(20000, 20400), 40, replace=False))  # seen everywhere
    vectors = []
    for k in range(n_kf):
        p = k % n_places
        n = int(rng.integers(60, 151))
        own = rng.choice(pools[p], int(n * 0.7), replace=False)
        nxt = rng.choice(pools[(p + 1) % n_places], int(n * 0.2), replace=False)
        com = rng.choice(shared, n - len(own) - len(nxt), replace=False)
        w = np.unique(np.concatenate([own, nxt, com])).astype(np.uint32)
        if k in (45, 75, 100):  # a view that shares no word with any other: no candidate
            w = (30000 + 200 * k + np.sort(rng.choice(200, n, replace=False))).astype(np.uint32)
        x = rng.uniform(0.2, 3.0, len(w))
        norm = 0.0
        for a in x:
            norm += abs(float(a))
        vectors.append((w, np.array([float(a) / norm for a in x], np.float64)))
    weight = {}
    for k in range(n_kf):
        for j in range(max(0, k - 6), k):
            weight[(j, k)] = int(rng.integers(5, 120)) // (k - j)
    erase_at = {int(k): int(k) - int(rng.integers(2, 5))
                for k in rng.choice(np.arange(20, n_kf), 6, replace=False)}
    steps, bad = [], np.zeros(n_kf, np.uint8)
    for k in range(n_kf):
        er = []
        if k in erase_at:
            bad[erase_at[k]] = 1
            er.append(erase_at[k])
        ordered, conn = [[] for _ in range(n_kf)], [[] for _ in range(n_kf)]
        for (a, b), wt in weight.items():
            if b > k or wt < 1:
                continue
            conn[a].append(b)
            conn[b].append(a)
            if wt >= 15:
                ordered[a].append((wt, b))
                ordered[b].append((wt, a))
        ordered = [[i for _, i in sorted(o, key=lambda t: (-t[0], t[1]))] for o in ordered]
        steps.append(dict(graph=dict(ordered=ordered, conn=conn, bad=bad.copy().tolist()),
                          erase=er))
    return vectors, steps


def run_scenario(d, vectors, steps, on_step=None):
    """DetectLoop for every keyframe with mLastLoopKFid = 0 -> [result per keyframe]."""
    out = []
    for k, st in enumerate(steps):
        d.set_bow(k, *vectors[k])
        for e in st["erase"]:
            d.db_erase(e)
        r = d.detect_loop(k, 0, st["graph"])
        r["groups"] = [(list(m), int(c)) for m, c in d.groups]
        out.append(r)
        if on_step:
            on_step(k, r)
    return out


def order_case(n=300, seed=4):
    """A query and a stored vector with all n words common and values over many binades.  The seed
    is one at which the reversed, the pairwise and the lane-strided sums all differ in bits from the
    sequential one, for L1 and L2 (test_loop_detect_ref_py.py asserts it)."""
    rng = np.random.default_rng(seed)
    w = np.sort(rng.choice(100000, n, replace=False)).astype(np.uint32)
    a = rng.uniform(0.5, 1.0, n) * 2.0 ** rng.integers(-40, 1, n)
    b = rng.uniform(0.5, 1.0, n) * 2.0 ** rng.integers(-40, 1, n)
    return w, a, b
