"""GPU parity of loop detection (mmt_loop_*, mmt_detect_loop_candidates, mmt_detect_loop:
k_loop_score plus the host logic of csrc/mmt_loopdetect.cpp) against the restatement
tests/loop_detect_ref_py.py.  Everything is compared exactly: counts, indices and orders as
integers, sums and scores as the bits of their doubles, minScore as the bits of its float.

Shapes are the smallest at which the kernel can go wrong: stored vectors around multiples of the
64-word step (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257) and a long one, queries of 1, 64,
65, 2000 and
MMT_LOOP_MAX_WORDS words, stored counts around the waves per workgroup (4) and past one workgroup
row (257), a common word in each step's first and last lane."""
import functools
import os
import struct

import numpy as np
import pytest

import loop_detect_cases as C
import loop_detect_ref_py as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
WAVES_PER_WG = 4  # kLoopWavesPerWG (csrc/mmt_loop.h)


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(nfeatures=2000))
    yield c
    c.close()


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class GpuLoop:
    """The library behind the interface of loop_detect_ref_py.RefLoop."""

    def __init__(self, ctx, scoring=0):
        self.ctx = ctx
        ctx.loop_reset(scoring)

    def set_bow(self, kf, words, values):
        self.ctx.loop_set_bow(kf, words, values)

    def db_add(self, kf):
        self.ctx.loop_db_add(kf)

    def db_erase(self, kf):
        self.ctx.loop_db_erase(kf)

    def score(self, q, k):
        s = self.ctx.loop_scores(q)
        return float(s["score"][s["ids"].tolist().index(k)])

    def candidates(self, kf, min_score, graph):
        return self.ctx.detect_loop_candidates(kf, min_score, graph)

    def detect_loop(self, kf, last_loop_kf_id, graph, consistency_th=3):
        return self.ctx.detect_loop(kf, last_loop_kf_id, graph, consistency_th)

    @property
    def groups(self):
        return self.ctx.loop_groups()


def normalised(rng, n):
    x = rng.uniform(0.1, 4.0, n)
    norm = 0.0
    for a in x:
        norm += abs(float(a))
    return np.array([float(a) / norm for a in x], np.float64)


def check_scores(ctx, q, vecs, scoring, ids=None):
    """loop_scores(q) against the restatement for every stored vector; returns the library's."""
    s = ctx.loop_scores(q)
    ids = list(vecs) if ids is None else ids
    assert s["ids"].tolist() == ids
    ref = [R.triple(*vecs[q], *vecs[k], scoring) for k in ids]
    assert s["common"].tolist() == [r[0] for r in ref]
    assert s["first"].tolist() == [r[1] for r in ref]
    rs = np.array([r[2] for r in ref], np.float64)
    assert np.array_equal(u64(s["sum"]), u64(rs)), np.nonzero(u64(s["sum"]) != u64(rs))[0][:10]
    rf = np.array([R.finish(r[2], scoring) for r in ref], np.float64)
    assert np.array_equal(u64(s["score"]), u64(rf))
    return s


@functools.lru_cache(maxsize=None)
def score_vectors():
    """id -> (words, values).  Query words are even, the others odd.  Queries (ids 100..) are
    nested prefixes-by-choice of one base of MMT_LOOP_MAX_WORDS even words."""
    import multimot_track_amd as M
    rng = np.random.default_rng(11)
    base = np.sort(rng.choice(60000, M.MMT_LOOP_MAX_WORDS, replace=False)).astype(np.uint32) * 2
    odd = np.arange(1, 120001, 2, dtype=np.uint32)
    q2000 = np.sort(rng.choice(base, 2000, replace=False))
    q65 = np.sort(rng.choice(q2000, 65, replace=False))
    q64 = q65[:64]
    vecs = {}
    # half query words, half not
    for i, n in enumerate([0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 2000]):
        nq = (n + 1) // 2
        w = np.concatenate([rng.choice(q2000, nq, replace=False),
                            rng.choice(odd, n - nq, replace=False)])
        vecs[i] = (np.sort(w).astype(np.uint32), normalised(rng, n))
    vecs[20] = (np.sort(rng.choice(odd, 200, replace=False)), normalised(rng, 200))  # none common
    w = np.concatenate([q2000[:1], rng.choice(odd, 99, replace=False)])
    vecs[21] = (np.sort(w), normalised(rng, 100))            # one common word: query index 0
    w = np.concatenate([q2000[-1:], rng.choice(odd, 99, replace=False)])
    vecs[22] = (np.sort(w), normalised(rng, 100))            # one: the last query index
    # 256 words, the query's at the first and last lane of every 64-word step (indices 0, 63, 64,
    # 127, ...), 62 odd words between the two of a step
    parts = []
    for j in range(4):
        lo, hi = int(q2000[400 * j]), int(q2000[400 * j + 200])
        between = np.arange(lo + 1, hi, dtype=np.uint32)
        between = between[between % 2 == 1]
        parts += [[lo], np.sort(rng.choice(between, 62, replace=False)), [hi]]
    w = np.concatenate(parts).astype(np.uint32)
    assert len(w) == 256 and np.all(np.diff(w.astype(np.int64)) > 0)
    assert all(int(w[p]) in set(q2000.tolist()) for p in (0, 63, 64, 127, 128, 191, 192, 255))
    vecs[23] = (w, normalised(rng, 256))
    for qid, qw in ((100, q2000[7:8]), (101, q64), (102, q65), (103, q2000), (104, base)):
        vecs[qid] = (np.ascontiguousarray(qw, np.uint32), normalised(rng, len(qw)))
    return vecs


@pytest.mark.parametrize("scoring", [0, 1], ids=["L1", "L2"])
def test_scores_match_restatement(ctx, scoring):
    import multimot_track_amd as M
    vecs = score_vectors()
    ctx.loop_reset(scoring)
    for k, (w, x) in vecs.items():
        ctx.loop_set_bow(k, w, x)
    ids = list(vecs)
    for q in (100, 101, 102, 103, 104):
        s = check_scores(ctx, q, vecs, scoring)
        assert s["common"][ids.index(q)] == len(vecs[q][0])  # all words common
        if q == 103:
            at = {k: ids.index(k) for k in (0, 20, 21, 22, 23)}
            assert (s["common"][at[0]], s["first"][at[0]], s["sum"][at[0]]) == (0, R.INT_MAX, 0.0)
            assert (s["common"][at[20]], s["first"][at[20]]) == (0, R.INT_MAX)
            assert (s["common"][at[21]], s["first"][at[21]]) == (1, 0)
            assert (s["common"][at[22]], s["first"][at[22]]) == (1, 1999)
            assert s["common"][at[23]] == 8
    # an empty stored vector as the query: nothing in common with anything
    s = check_scores(ctx, 0, vecs, scoring)
    assert not s["common"].any()
    # one word more than the bound
    n = M.MMT_LOOP_MAX_WORDS + 1
    with pytest.raises(M.MmtError, match="-22"):
        ctx.loop_set_bow(200, np.arange(n, dtype=np.uint32), np.full(n, 1.0 / n))
    assert ctx.loop_stats()["n_stored"] == len(vecs)


def test_stored_counts_round_the_workgroup(ctx):
    rng = np.random.default_rng(12)
    pool = np.sort(rng.choice(5000, 400, replace=False)).astype(np.uint32)
    vecs = {}
    ctx.loop_reset(0)
    for k in range(257):
        n = int(rng.integers(40, 100))
        vecs[k] = (np.sort(rng.choice(pool, n, replace=False)), normalised(rng, n))
        ctx.loop_set_bow(k, *vecs[k])
        if k + 1 in (1, WAVES_PER_WG - 1, WAVES_PER_WG, WAVES_PER_WG + 1, 257):
            check_scores(ctx, k, vecs, 0)
            check_scores(ctx, 0, vecs, 0)


@pytest.mark.parametrize("scoring", [0, 1], ids=["L1", "L2"])
def test_sum_is_sequential(ctx, scoring):
    """The order case: values over many binades, where the reversed, pairwise and lane-strided
    sums all differ from the sequential one (test_loop_detect_ref_py.py): the kernel's is the
    sequential one."""
    w, a, b = C.order_case()
    ctx.loop_reset(scoring)
    ctx.loop_set_bow(0, w, a)
    ctx.loop_set_bow(1, w, b)
    s = ctx.loop_scores(0)
    terms = [x for _, _, x in R.common_terms(w, a, w, b, scoring)]
    seq = R.sum_sequential(terms)
    print("kernel %r sequential %r reversed %r pairwise %r" % (
        float(s["sum"][1]), seq, R.sum_reversed(terms), R.sum_pairwise(terms)))
    assert struct.pack("<d", s["sum"][1]) == struct.pack("<d", seq)
    assert s["common"][1] == len(w) and s["first"][1] == 0


def test_growth_keeps_stored_vectors(ctx):
    rng = np.random.default_rng(13)
    pool = np.sort(rng.choice(200000, 6000, replace=False)).astype(np.uint32)
    vecs = {}
    ctx.loop_reset(0)
    for k in range(3):
        vecs[k] = (np.sort(rng.choice(pool, 2000, replace=False)), normalised(rng, 2000))
        ctx.loop_set_bow(k, *vecs[k])
    before = check_scores(ctx, 0, vecs, 0)
    st0 = ctx.loop_stats()
    assert st0["word_grown"] == 0 and st0["value_grown"] == 0
    k = 3
    while min(ctx.loop_stats()["word_grown"], ctx.loop_stats()["value_grown"]) < 2:
        assert k < 200
        vecs[k] = (np.sort(rng.choice(pool, 2000, replace=False)), normalised(rng, 2000))
        ctx.loop_set_bow(k, *vecs[k])
        k += 1
    st = ctx.loop_stats()
    print(st0, st)
    assert st["word_capacity"] >= 4 * st0["word_capacity"] and st["n_stored"] == k
    assert st["value_capacity"] >= 4 * st0["value_capacity"]
    assert st["word_capacity"] >= 2000 * k
    after = ctx.loop_scores(0)  # the query is the first stored vector
    for f in ("common", "first"):
        assert np.array_equal(after[f][:3], before[f])
    assert np.array_equal(u64(after["sum"][:3]), u64(before["sum"]))
    assert np.array_equal(u64(after["score"][:3]), u64(before["score"]))
    check_scores(ctx, k - 1, vecs, 0)


@pytest.mark.parametrize("case", C.HAND_CASES, ids=lambda f: f.__name__)
def test_hand_case(ctx, case):
    case(lambda scoring: GpuLoop(ctx, scoring))


def test_reset_and_errors(ctx):
    import multimot_track_amd as M
    d = GpuLoop(ctx, 0)
    for k, (w, v) in C.ORDER_VECS.items():
        d.set_bow(k, w, v)
    for k in range(4):
        d.db_add(k)
    g = C.graph(5)
    assert d.candidates(4, 0.0, g) == [1, 3, 0, 2]
    st = ctx.loop_stats()
    assert (st["n_stored"], st["n_members"]) == (5, 4)

    def einval(f, *a):
        with pytest.raises(M.MmtError, match="-22"):
            f(*a)

    einval(d.db_add, 77)                     # an unknown id
    einval(d.db_erase, 77)
    einval(ctx.loop_scores, 77)
    einval(d.candidates, 77, 0.0, g)
    einval(d.db_add, 2)                      # a second add
    einval(d.set_bow, 2, [1], [1.0])         # a second set_bow
    einval(d.set_bow, 9, [3, 3], [0.5, 0.5])  # not strictly ascending
    einval(d.set_bow, 9, [4, 3], [0.5, 0.5])
    einval(d.candidates, 4, 0.0, C.graph(4))  # the graph is too small for the query
    einval(d.candidates, 4, 0.0, C.graph(5, conn={4: [5]}))  # a listed id outside the graph
    einval(ctx.loop_reset, 2)
    assert d.candidates(4, 0.0, g) == [1, 3, 0, 2]  # nothing changed, the context still works
    # DetectLoop: a non-bad covisible keyframe with no stored vector; bad, it is skipped
    d.set_bow(10, [10, 20], [0.5, 0.5])
    einval(d.detect_loop, 10, 0, C.graph(11, ordered={10: [6]}, conn={10: [6]}))
    assert ctx.loop_stats()["n_members"] == 4 and d.groups == []
    einval(d.detect_loop, 10, 0, C.graph(10))  # the graph is too small
    r = d.detect_loop(10, 0, C.graph(11, ordered={10: [6]}, conn={10: [6]}, bad=[6]))
    assert r["ran"] and r["candidates"] == [] and ctx.loop_stats()["n_members"] == 5
    einval(d.detect_loop, 10, 0, C.graph(11))  # a member already
    # reset empties everything
    einval(d.detect_loop, 4, -100, g)  # keyframe 10 is in the database and outside this graph
    r = d.detect_loop(4, -100, C.graph(11))
    assert r["candidates"] == [10] and d.groups == [([10], 0)]  # the identical keyframe 10
    ctx.loop_reset(0)
    st = ctx.loop_stats()
    assert (st["n_stored"], st["n_members"], st["word_capacity"], st["value_capacity"],
            st["word_grown"], st["value_grown"]) == (0, 0, 0, 0, 0, 0)
    assert d.groups == []
    einval(ctx.loop_scores, 4)
    d.set_bow(4, [10, 20], [0.5, 0.5])  # ids are free again
    assert d.candidates(4, 0.0, g) == []


@functools.lru_cache(maxsize=None)
def scenario_reference():
    vectors, steps = C.scenario()
    return vectors, steps, C.run_scenario(R.RefLoop(0, False), vectors, steps)


def test_scenario_end_to_end(ctx):
    vectors, steps, ref = scenario_reference()
    got = C.run_scenario(GpuLoop(ctx, 0), vectors, steps)
    assert len(got) == len(ref) == 120
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a["ran"] == b["ran"], k
        assert np.float32(a["min_score"]).tobytes() == np.float32(b["min_score"]).tobytes(), k
        assert a["candidates"] == b["candidates"], k
        assert a["enough"] == b["enough"], k
        assert a["n_groups"] == b["n_groups"], k
        assert a["groups"] == b["groups"], k
    st = ctx.loop_stats()
    assert st["n_stored"] == 120
    assert st["n_members"] == 120 - len({e for s in steps for e in s["erase"]})


def bow_vector(word, weight):
    """DBoW2's transform as DESIGN section 2 states it: the weights of equal words added in feature
    order, the vector normalised by its L1 norm summed in word order."""
    acc = {}
    for w, x in zip(word.tolist(), weight.tolist()):
        if not x > 0:
            continue
        acc[w] = acc[w] + x if w in acc else x
    ws = sorted(acc)
    norm = 0.0
    for w in ws:
        norm += abs(acc[w])
    return np.array(ws, np.uint32), np.array([acc[w] / norm for w in ws], np.float64)


def test_from_descriptors(ctx):
    voc = os.path.join(HERE, "golden", "test_voc_k10l6.txt")
    with open(voc) as f:
        scoring = int(f.readline().split()[2])
    assert scoring == 0  # L1, the normalisation bow_vector applies
    ctx.load_vocabulary(voc)
    rng = np.random.default_rng(14)
    images = [rng.integers(0, 256, (300, 32), dtype=np.uint8) for _ in range(8)]
    for k in range(4):  # the later images: earlier ones with a few bits flipped
        d = images[k].copy()
        rows = rng.choice(300, 40, replace=False)
        d[rows, rng.integers(0, 32, 40)] ^= (1 << rng.integers(0, 8, 40)).astype(np.uint8)
        images.append(d)
    d = GpuLoop(ctx, scoring)
    ref = R.RefLoop(scoring, False)
    for k, desc in enumerate(images):
        word, weight, _ = ctx.bow_transform(desc)
        w, x = bow_vector(word, weight)
        assert 0 < len(w) <= 300
        for api in (d, ref):
            api.set_bow(k, w, x)
            if k < 8:
                api.db_add(k)
    g = C.graph(12)
    for k in range(8, 12):
        got = d.candidates(k, 0.0, g)
        print("image %d: candidates %s" % (k, got))
        assert got == ref.candidates(k, 0.0, g)
        assert got[0] == k - 8
