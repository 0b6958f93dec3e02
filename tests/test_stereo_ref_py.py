"""The sequential restatement of the stereo Frame constructor (tests/stereo_ref_py.py, from the
reference's Frame.cc:79-159 and :849-1038) against answers worked by hand and against image pairs
of known disparity.  CPU only.  tests/test_gpu_stereo.py then pins the kernels to the restatement,
bit for bit."""
import math

import numpy as np
import pytest

import orb_ref_py as R
import stereo_cases as C
import stereo_ref_py as S

F = np.float32


# ------------------------------------------------------------------ known answers
def test_row_ranges():
    """:873-875.  Level 0: r = 1.2f, a key at y = 100 is listed in floor(98.8) = 98 .. ceil(101.2)
    = 102.  Level 7: scale = 1.2f^7 = 3.5831816, r = 4.299818, floor(95.70) = 95 .. ceil(104.30)
    = 105.  An integer y - r or y + r adds no row: y = 1.2f at level 0 starts at row 0."""
    sc = R.config(500)["scale"]
    assert S.row_range(F(100), 0, sc) == (98, 102)
    assert S.row_range(F(100), 7, sc) == (95, 105)
    assert S.row_range(F(1.2), 0, sc) == (0, 3)
    k = np.zeros(2, R.KP_DTYPE)
    k["y"], k["octave"] = (100, 100), (0, 7)
    rows = S.row_table(k, sc, 240)
    assert [y for y in range(240) if 0 in rows[y]] == list(range(98, 103))
    assert [y for y in range(240) if 1 in rows[y]] == list(range(95, 106))
    assert rows[100] == [0, 1]  # ascending key order inside a row


def test_parabola():
    """:999.  (10, 4, 6): (10 - 6) / (2 * (10 + 6 - 8)) = 0.25.  A zero denominator: 0 / 0 is a NaN,
    which passes the delta test and fails the disparity range test; x / 0 is an infinity, which
    fails the delta test.  Either way no match."""
    assert S.parabola(10, 4, 6) == F(0.25)
    nan = S.parabola(5, 5, 5)
    assert math.isnan(nan)
    assert S.accept(100, F(1), 80, 0, nan, C.BF)[0] == "range"
    inf = S.parabola(6, 5, 4)
    assert math.isinf(inf)
    assert S.accept(100, F(1), 80, 0, inf, C.BF)[0] == "delta"


def test_delta_bounds_and_disparity_range():
    """:1001 keeps -1 and 1, rejects their neighbours; :1009 keeps [0, 200)."""
    up, dn = np.nextafter(F(1), F(2)), np.nextafter(F(-1), F(-2))
    assert S.accept(100, F(1), 80, 0, F(1), C.BF)[0] == "ok"
    assert S.accept(100, F(1), 80, 0, F(-1), C.BF)[0] == "ok"
    assert S.accept(100, F(1), 80, 0, up, C.BF)[0] == "delta"
    assert S.accept(100, F(1), 80, 0, dn, C.BF)[0] == "delta"
    # uL = 250: bestuR = 50 gives 200 (rejected), 50.5 gives 199.5; bestuR = 250.25 gives -0.25
    assert S.accept(250, F(1), 50, 0, F(0), C.BF)[0] == "range"
    st, u, z, cl = S.accept(250, F(1), 50, 0, F(0.5), C.BF)
    assert (st, u, z, cl) == ("ok", F(50.5), F(C.BF) / F(199.5), False)
    assert S.accept(250, F(1), 250, 0, F(0.25), C.BF)[0] == "range"
    # the level's scale factor multiplies the sum: 1.2f * (10 + 2 + 0.5) = 15.000001
    st, u, z, cl = S.accept(100, F(1.2), 10, 2, F(0.5), C.BF)
    assert u == F(1.2) * F(12.5) and z == F(C.BF) / (F(100) - u)


def test_clamp_at_zero_disparity():
    """:1011-1015: disparity 0 becomes (float)0.01 and bestuR = (float)(uL - 0.01)."""
    st, u, z, cl = S.accept(100, F(1), 100, 0, F(0), C.BF)
    assert st == "ok" and cl
    assert u == F(99.99) and z == F(C.BF) / F(0.01)


def test_round_half_away_from_zero():
    """C round(), not cvRound: 2.5 -> 3, -2.5 -> -3, 0.5 -> 1, -0.5 -> -1 (rint gives 2, -2, 0, 0)."""
    got = [float(S.c_round(v)) for v in (2.5, -2.5, 0.5, -0.5, 3.5, 2.4999998, -7.5, 0.0)]
    assert got == [3, -3, 1, -1, 4, 2, -8, 0]
    assert float(S.c_round(np.nextafter(F(0.5), F(0)))) == 0


def test_median_rule_equals_threshold_rule():
    """:1023-1037.  SADs (10, 4, 10, 21, 21, 22, 3): sorted 3 4 10 10 21 21 22, element [3] = 10,
    thDist = (1.5f * 1.4f) * 10 = 2.0999999f * 10 = 21.0f (the product lies midway between two
    floats and rounds to even), so both 21s tie with the threshold and go, with the 22."""
    pairs = [(10, 0), (4, 1), (10, 2), (21, 3), (21, 4), (22, 5), (3, 6)]
    assert S.median_threshold([p[0] for p in pairs]) == (10, F(21.0))
    assert sorted(S.median_clear_sorted(pairs)) == [3, 4, 5]
    assert sorted(S.median_clear_threshold(pairs)) == [3, 4, 5]
    # median 30: thDist = 62.999996f, a SAD of 63 goes
    pairs = [(30, 0), (63, 1), (1, 2)]
    assert S.median_threshold([30, 63, 1])[1] == F(62.999996)
    assert S.median_clear_sorted(pairs) == [1] == S.median_clear_threshold(pairs)
    # even sizes take the upper middle; one element is its own median; none: nothing (pin a)
    assert S.median_threshold([7, 9])[0] == 9 and S.median_threshold([7])[0] == 7
    assert S.median_threshold([]) == (-1, F(0)) and S.median_clear_sorted([]) == []
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = int(rng.integers(1, 40))
        pairs = [(int(d), i) for i, d in enumerate(rng.integers(0, 30, n))]
        assert sorted(S.median_clear_sorted(pairs)) == sorted(S.median_clear_threshold(pairs))


@pytest.mark.parametrize("subset", sorted(C.HAND_SUBSETS))
def test_hand_placed_keys(subset):
    """Every event the hand-placed keys of tests/stereo_cases.py were chosen for occurs in the
    restatement: the bestIdxR == 0 quirk, ties, the inclusive bounds, both thresholds, the border
    tests, the end shifts, deltaR = 0.5, the clamp, the range test at level 7, and accepted lists of
    0, 1 and 2 keys."""
    out = C.hand_reference(subset)
    C.hand_events(subset, out)
    c = out["counters"]
    assert c["n_coarse"] == (c["n_window_edge"] + c["n_end_shift"] + c["n_delta"] + c["n_range"] +
                             c["n_accepted"])


def test_refusals():
    """Pin (c): keys the reference would index out of bounds with."""
    c = C.hand_case("accepted1")
    cfg = R.config(500)
    pl, pr = R.pyramid(c["left"], cfg), R.pyramid(c["right"], cfg)

    def run(kl, kr):
        return S.stereo_matches(pl, pr, kl, c["dl"], kr, c["dr"], cfg["scale"], cfg["inv_scale"],
                                C.BF)
    for field, value in (("x", 3.0), ("octave", 8), ("y", 237.0)):
        kl = c["kl"].copy()
        kl[field][0] = value
        with pytest.raises(ValueError):
            run(kl, c["kr"])
    for field, value in (("y", 1.0), ("y", 238.5), ("octave", -1)):
        kr = c["kr"].copy()
        kr[field][0] = value
        with pytest.raises(ValueError):
            run(c["kl"], kr)


# ------------------------------------------------------------------ image pairs
def test_identical_pair_has_no_match():
    """Every SAD is 0, the median is 0, thDist is 0 and dist < 0 never holds: all 254 accepted keys
    of the crop [60:320, 400:800] of kitti_sample frame 0 (500 features) are cleared."""
    out = C.reference("crop_identical")
    c = out["counters"]
    assert c["n_accepted"] == 254 and c["n_median_removed"] == 254 and c["median"] == 0
    assert (out["uR"] == -1).all() and (out["depth"] == -1).all()
    # vDescIndex survives where the match failed the range test (:944 comes before the refinement)
    ri = out["right_idx"]
    assert ((ri == -1) | (ri == np.arange(len(ri)))).all() and 0 < (ri >= 0).sum() <= c["n_range"]


# Measured with this restatement on the crop (509 left keys): survivors, worst error in level px
#   shift 12, noise 3:  259, 0.46      shift 37, none: 292, 0.72      shift 150, noise 3: 210, 0.67
@pytest.mark.parametrize("name,d,floor", [("crop_s12_n3", 12, 130), ("crop_s37_n0", 37, 146),
                                          ("crop_s150_n3", 150, 105)])
def test_shifted_pair(name, d, floor):
    """The right image is the left one shifted by d columns (plus uniform +-3 grey noise): every
    surviving key's disparity lies within one level pixel of d, and at least half of the measured
    survivors (above) survive."""
    out = C.reference(name)
    k = C.stages(name, 0)["kps"]
    scale = np.array(C.stages(name, 0)["cfg"]["scale"], F)
    ok = out["uR"] >= 0
    err = np.abs((k["x"] - out["uR"])[ok] - d) / scale[k["octave"][ok]]
    print("%s: %d left keys, %d survivors, worst error %.3f level px, counters %s" %
          (name, len(k), ok.sum(), err.max(), out["counters"]))
    assert ok.sum() >= floor
    assert (err <= 1).all()
    assert (out["depth"][ok] == F(C.BF) / (k["x"] - out["uR"])[ok]).all()
    assert ((out["depth"] == -1) == ~ok).all()


def test_stereo_frame_early_return_and_labels():
    """:103 an image without a key returns early with the right count reported; :116-124 the label
    is the mask at the truncated coordinates."""
    flat = np.full((260, 400), 90, np.uint8)
    out = S.stereo_frame(flat, C.crop(), nfeatures=500)
    assert len(out["kps"]) == 0 and len(out["uR"]) == 0 and len(out["kps_right"]) == 509
    mask = (np.arange(260)[:, None] * 1000 + np.arange(400)[None, :]).astype(np.int32)
    out = S.stereo_frame(C.crop(), C.crop(), mask, nfeatures=500)
    k = out["kps"]
    assert (out["sem_label"] == k["y"].astype(np.int64) * 1000 + k["x"].astype(np.int64)).all()
