"""Pins of the restatement tests/bow_kf_ref_py.py (SearchByBoW(KeyFrame*, KeyFrame*),
ORBmatcher.cc:897-1030) to facts that do not depend on it: hand-built cases of a few keys whose
outcome follows from the reference's text by hand, and a cross-check against the C++ oracle of C4
(SearchByBoW(KeyFrame*, Frame&)), which computes the same matches wherever every key of side 2
holds a MapPoint and no best distance is exactly TH_LOW (C4 accepts <= 50, this one < 50)."""
import numpy as np
import pytest

import bow_kf_problems as KP
import bow_kf_ref_py as RK
from bow_kf_problems import bits, hand


def run(kf1, kf2, **kw):
    kw.setdefault("check_orientation", False)
    nm, m, tr = RK.search_by_bow_kf(kf1, kf2, literal=True, **kw)
    nm_f, m_f, tr_f = RK.search_by_bow_kf(kf1, kf2, literal=False, **kw)
    assert nm == nm_f and np.array_equal(m, m_f) and tr == tr_f
    return nm, m.tolist(), tr


def test_distance_49_is_accepted_and_50_is_not():
    nm, m, tr = run(*KP.case_49_50())
    assert tr[0] == (49, 256, 0) and tr[1] == (50, 256, 1)
    assert m == [0, -1] and nm == 1


def test_key_without_mappoint_is_neither_matched_nor_counted():
    kf1, kf2 = KP.case_no_mappoint()
    nm, m, tr = run(kf1, kf2)
    assert tr[0] == (30, 256, 1) and m == [1] and nm == 1
    # with all three MapPoints the closest key wins
    all_ok = (kf2[0], kf2[1], kf2[2], np.ones(3, np.uint8))
    nm, m, tr = run(kf1, all_ok)
    assert tr[0] == (10, 30, 0) and m == [0]
    # and with key 2's alone the ratio test fails: 30 < 0.75 * 35 = 26.25 is false
    two = (kf2[0], kf2[1], kf2[2], np.array([0, 1, 1], np.uint8))
    nm, m, tr = run(kf1, two)
    assert tr[0] == (30, 35, 1) and m == [-1] and nm == 0


@pytest.mark.parametrize("second,accepted", [(40, False), (41, True)])
def test_ratio_test_is_strict_in_float(second, accepted):
    """30 < 0.75f * 40 = 30.0 is false; 30 < 0.75f * 41 = 30.75 is true."""
    kf1 = hand([bits()], {0: [0]})
    kf2 = hand([bits(range(second)), bits(range(30))], {0: [0, 1]})
    nm, m, tr = run(kf1, kf2, nnratio=0.75)
    assert tr[0] == (30, second, 1)
    assert m == ([1] if accepted else [-1]) and nm == int(accepted)


def test_first_of_equal_distances_in_list_order_wins():
    """Keys 0 and 1 of keyframe 2 both at distance 20, listed as [1, 0]: key 1 is seen first and
    '<' keeps it.  bestDist2 is 20 too (ties count), so only a ratio above 1 lets it through."""
    kf1 = hand([bits()], {6: [0]})
    kf2 = hand([bits(range(20)), bits(range(100, 120)), bits(range(60))], {6: [1, 0, 2]})
    nm, m, tr = run(kf1, kf2, nnratio=1.5)
    assert tr[0] == (20, 20, 1) and m == [1] and nm == 1
    nm, m, tr = run(kf1, kf2, nnratio=0.75)
    assert tr[0] == (20, 20, 1) and m == [-1] and nm == 0
    kf2 = hand(list(kf2[2]), {6: [0, 1, 2]})
    assert run(kf1, kf2, nnratio=1.5)[1] == [0]


@pytest.mark.parametrize("with_next_best", [True, False])
def test_first_key_in_list_order_takes_the_shared_best(with_next_best):
    """Keys A (index 1) and B (index 0) of keyframe 1, listed as [A, B], are both closest to key X
    of keyframe 2 (distances 2 and 3).  A replays first and takes X; B then sees only Y, 30 away
    (accepted: nothing else is left, bestDist2 = 256), or nothing."""
    A, B = bits(), bits(range(5))
    X, Y = bits(range(2)), bits(range(5), range(100, 130))
    kf1 = hand([B, A], {3: [1, 0]})
    kf2 = hand([X, Y] if with_next_best else [X], {3: [0, 1] if with_next_best else [0]})
    nm, m, tr = run(kf1, kf2)
    if with_next_best:
        assert tr[1] == (2, 35, 0) and tr[0] == (30, 256, 1)
        assert m == [1, 0] and nm == 2
    else:
        assert tr[1] == (2, 256, 0) and tr[0] == (256, 256, -1)
        assert m == [-1, 0] and nm == 1


def test_nodes_on_one_side_only_are_skipped():
    z = bits()
    kf1 = hand([z, z, z], {1: [0], 5: [1], 9: [2]})
    kf2 = hand([z, z, z, z], {2: [0], 5: [1], 7: [2], 9: [3]})
    nm, m, tr = run(kf1, kf2)
    assert m == [-1, 1, 3] and nm == 2 and sorted(tr) == [1, 2]
    nm, m, tr = run(kf2, kf1)
    assert m == [-1, 1, -1, 2] and nm == 2


def test_compute_three_maxima():
    def h(**bins):
        s = [0] * RK.HISTO_LENGTH
        for k, v in bins.items():
            s[int(k[1:])] = v
        return s
    assert RK.compute_three_maxima(h(b3=50, b7=20, b11=10, b20=6)) == (3, 7, 11)
    assert RK.compute_three_maxima(h(b3=50, b7=20, b11=4)) == (3, 7, -1)   # 4 < 5
    assert RK.compute_three_maxima(h(b3=50, b7=5, b11=5)) == (3, 7, 11)    # 5 < 5 is false
    assert RK.compute_three_maxima(h(b3=50, b7=4, b11=3)) == (3, -1, -1)
    assert RK.compute_three_maxima(h(b11=7, b3=7, b7=7)) == (3, 7, 11)     # '>' keeps the first
    assert RK.compute_three_maxima(h()) == (-1, -1, -1)


@pytest.mark.parametrize("n_main,removed", [(11, 1), (10, 0)])
def test_rotation_filter_drops_bins_below_a_tenth(n_main, removed):
    """n_main matches turned by 0 degrees (bin 0) and one by 90 (bin round(90 / 30) = 3): the single
    one goes when 1 < 0.1 * n_main, that is from 11 on."""
    n = n_main + 1
    z = bits()
    kf1 = hand([z] * n, {k: [k] for k in range(n)}, angle=[100.0] * n_main + [100.0])
    kf2 = hand([z] * n, {k: [k] for k in range(n)}, angle=[100.0] * n_main + [10.0])
    nm, m, tr = run(kf1, kf2, check_orientation=True)
    assert nm == n - removed
    assert m[:n_main] == list(range(n_main)) and m[n_main] == (-1 if removed else n_main)
    # a negative difference wraps: 10 - 100 + 360 = 270 -> bin 9
    nm, m, tr = run(kf2, kf1, check_orientation=True)
    assert nm == n - removed


def test_scan_fast_equals_scan_loop():
    rng = np.random.default_rng(3)
    for n in (0, 1, 2, 3, 17, 300):
        for hi in (3, 40, 257):
            d = rng.integers(0, hi, n).astype(np.int32)
            idx = rng.permutation(n)
            assert RK.scan_fast(d, idx) == RK.scan_loop(d, idx)


# ---------------------------------------------------------------------------- the C++ oracle
# seeds on which every MapPoint flag of side 2 is 1 and no replayed feature has bestDist1 == 50
SMALL = dict(n_kf=300, n_f=400, n_nodes=25, mp_valid2=1.0)
CLEAN = [(35, {}), (40, {"shuffle": True}), (48, {"dup": 0.3, "rot_outliers": 0.5})]


def as_c4(nm, match12, n2):
    """match12 (key of keyframe 1 -> key of keyframe 2) in C4's direction."""
    m = np.full(n2, -1, np.int32)
    i1 = np.nonzero(match12 >= 0)[0]
    m[match12[i1]] = i1
    return nm, m


@pytest.mark.parametrize("seed,kw", CLEAN)
@pytest.mark.parametrize("ratio,orient", [(0.75, True), (0.7, False)])
def test_equals_c4_oracle_where_the_two_coincide(oracle_mod, seed, kw, ratio, orient):
    kf1, kf2 = KP.kf_problem(seed, **SMALL, **kw)
    assert kf2[3].all()
    nm, m12, tr = RK.search_by_bow_kf(kf1, kf2, ratio, orient)
    assert all(t[0] != RK.TH_LOW for t in tr.values())
    assert nm > 20
    nm_o, m_o = oracle_mod.search_by_bow(*kf1, *kf2[:3], nnratio=ratio, check_orientation=orient)
    nm_c, m_c = as_c4(nm, m12, len(kf2[1]))
    assert nm_c == nm_o and np.array_equal(m_c, m_o)


def test_differs_from_c4_oracle_in_the_key_at_distance_50(oracle_mod):
    """A clean seed plus one node of its own holding one pair at distance exactly 50, turned like
    the rest: C4 takes it (50 <= TH_LOW), SearchByBoW(KeyFrame*, KeyFrame*) does not."""
    (fv1, k1, d1, ok1), (fv2, k2, d2, ok2) = KP.kf_problem(35, **SMALL)
    rng = np.random.default_rng(9)
    new1, new2 = len(k1), len(k2)
    extra1, extra2 = k1[:1].copy(), k2[:1].copy()
    extra1["angle"], extra2["angle"] = 100.0, 88.0  # the problem's rotation of 12 degrees
    k1, k2 = np.concatenate([k1, extra1]), np.concatenate([k2, extra2])
    d1 = np.concatenate([d1, rng.integers(0, 256, (1, 32), dtype=np.uint8)])
    d2 = np.concatenate([d2, KP.flip_bits(rng, d1[-1], 50)[None]])
    ok1, ok2 = np.append(ok1, 1).astype(np.uint8), np.append(ok2, 1).astype(np.uint8)
    node = int(max(fv1[0].max(), fv2[0].max())) + 1

    def grow(fv, key):
        return (np.append(fv[0], node).astype(np.uint32),
                np.append(fv[1], fv[1][-1] + 1).astype(np.int32),
                np.append(fv[2], key).astype(np.int32))
    kf1, kf2 = (grow(fv1, new1), k1, d1, ok1), (grow(fv2, new2), k2, d2, ok2)
    nm, m12, tr = RK.search_by_bow_kf(kf1, kf2, 0.75, True)
    assert [i for i, t in tr.items() if t[0] == RK.TH_LOW] == [new1]
    assert tr[new1] == (50, 256, new2) and m12[new1] == -1
    nm_o, m_o = oracle_mod.search_by_bow(*kf1, *kf2[:3], nnratio=0.75, check_orientation=True)
    nm_c, m_c = as_c4(nm, m12, len(k2))
    assert nm_o == nm_c + 1
    assert np.nonzero(m_c != m_o)[0].tolist() == [new2] and m_o[new2] == new1
