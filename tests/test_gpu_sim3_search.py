"""ORBmatcher::SearchBySim3 on the GPU (mmt_search_by_sim3: k_sim3_search for both directions and
the host's agreement pass) against the NumPy restatement tests/sim3_ref_py.py: vnMatch1, vnMatch2,
the new matches and the return value are bit for bit the restatement's."""
import numpy as np
import pytest

import sim3_cases as C
import sim3_ref_py as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(nfeatures=2000))
    yield c
    c.close()


@pytest.fixture(scope="module")
def scale(ctx):
    s, _ = C.orb_scales()
    assert np.array_equal(np.asarray(ctx.levels()["scale"], np.float32)[:len(s)], s)
    return s


def check(ctx, scale, kf1, kf2, sim3, matched=None, th=7.5):
    n1 = len(kf1["skip"])
    m = np.full(n1, -1, np.int32) if matched is None else matched
    ref = R.search_by_sim3(kf1, kf2, sim3["s"], sim3["R"], sim3["t"], th, m, C.K_KITTI, C.W, C.H,
                           scale)
    nf, match, c1, c2 = ctx.search_by_sim3(kf1, kf2, sim3["s"], sim3["R"], sim3["t"], th, m)
    assert np.array_equal(c1, ref["cand1"])
    assert np.array_equal(c2, ref["cand2"])
    assert np.array_equal(match, ref["match"])
    assert nf == ref["n_found"]
    return ref


@pytest.mark.parametrize("s12", [1.0, 1.15, 0.9])
def test_keyframe_pair_recovers_the_mutual_matches(ctx, scale, s12):
    kf1, kf2, sim3, pair = C.keyframe_pair(11, 220, s12=s12)  # 300 keys a side
    ref = check(ctx, scale, kf1, kf2, sim3)
    assert np.array_equal(ref["match"][:len(pair)], pair) and ref["n_found"] == len(pair)


@pytest.mark.parametrize("s12", [1.0, 1.15])
def test_edge_cases_and_prior_matches(ctx, scale, s12):
    kf1, kf2, sim3, matched = C.edge_case(12, 220, s12)
    ref = check(ctx, scale, kf1, kf2, sim3, matched)
    r = ref["reasons1"]
    assert [r[i] for i in (3, 4, 5)] == ["behind", "outside", "distance"]
    assert r[6] in ("octave", "far") and r[8] in ("empty", "octave", "far")
    assert all(r[i] == "matched" for i in range(10, 30))
    n2 = len(kf2["skip"])
    assert np.any(ref["cand1"] >= n2 - 4)  # a twin key won its tie ...
    assert ref["n_found"] < 220 - 25       # ... and the pair was dropped with the skipped ones


def test_other_window_sizes(ctx, scale):
    kf1, kf2, sim3, _ = C.keyframe_pair(13, 220, s12=1.05)
    for th in (3.0, 15.0):
        check(ctx, scale, kf1, kf2, sim3, th=th)


def test_two_thousand_keys(ctx, scale):
    kf1, kf2, sim3, pair = C.keyframe_pair(14, 1500, n_only=250, n_empty=250, s12=1.1)
    ref = check(ctx, scale, kf1, kf2, sim3)
    assert ref["n_found"] > 1400


def test_empty_and_bad_arguments(ctx, scale):
    import multimot_track_amd as M
    kf1, kf2, sim3, _ = C.keyframe_pair(15, 30, n_only=5, n_empty=5)
    none = C.copy_kf(kf1)
    none["skip"][:] = 1
    ref = check(ctx, scale, none, kf2, sim3)
    assert ref["n_found"] == 0
    bad = C.copy_kf(kf1)
    bad["skip"] = bad["skip"][:-1]
    with pytest.raises(ValueError):
        ctx.search_by_sim3(bad, kf2, sim3["s"], sim3["R"], sim3["t"])
    out = C.copy_kf(kf1)
    out["kps"]["octave"][0] = 9
    with pytest.raises(M.MmtError):
        ctx.search_by_sim3(out, kf2, sim3["s"], sim3["R"], sim3["t"])
