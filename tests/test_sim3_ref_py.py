"""The NumPy restatement of Sim3Solver and SearchBySim3 (tests/sim3_ref_py.py) pinned to facts that
do not depend on it: known similarities are recovered, T12 T21 = I, an all-inlier minimal set counts
every inlier, SetRansacParameters' iteration caps, the identical-sets NaN case, and for
SearchBySim3 synthetic keyframe pairs whose mutual matches are known by construction, with one
point per skip reason."""
import numpy as np
import pytest

import sim3_cases as C
import sim3_ref_py as R

f32 = np.float32


def spread_triple(X):
    """Three well-spread points: the farthest pair and the point farthest from their line."""
    d = np.linalg.norm(X[:, None] - X[None], axis=2)
    a, b = np.unravel_index(np.argmax(d), d.shape)
    ab = (X[b] - X[a]) / d[a, b]
    off = np.linalg.norm(np.cross(X - X[a], ab), axis=1)
    return [int(a), int(b), int(np.argmax(off))]


@pytest.mark.parametrize("fix_scale", [True, False])
def test_noise_free_points_recover_the_similarity(fix_scale):
    for seed in range(4):
        p = C.solver_problem(seed, 40, 0.0, 0.0, fix_scale)
        tr = p["truth"]
        idx = spread_triple(p["X1"].astype(np.float64))
        h = R.compute_sim3(p["X1"][idx].T, p["X2"][idx].T, fix_scale)
        assert np.abs(h["R"] - tr["R"]).max() < 1e-4
        assert np.abs(h["t"] - tr["t"]).max() < 1e-4
        assert abs(float(h["s"]) - tr["s"]) < 1e-4
        assert np.abs(h["T12"].astype(np.float64) @ h["T21"].astype(np.float64) -
                      np.eye(4)).max() < 1e-5


def test_hypothesis_from_three_inliers_counts_every_inlier():
    p = C.solver_problem(5, 200, 0.4, 0.0, False)
    S = R.Sim3Solver(p["X1"], p["X2"], p["sigma2_1"], p["sigma2_2"], p["K1"], p["K2"], False)
    inl = np.flatnonzero(p["truth"]["inliers"])
    # draws that select three inliers through the swap-with-back removal: ascending indices from
    # the front are never displaced
    h = S.hypothesis(inl[:3])
    assert h["idx"] == list(inl[:3])
    assert np.all(h["mask"][inl])
    assert h["count"] >= len(inl)


def test_iteration_caps():
    got = [R.ransac_max_iterations(n, 0.99, 20, 300) for n in (19, 20, 21, 25, 40, 100, 400)]
    assert got == [1, 1, 3, 7, 35, 300, 300]


def test_too_few_correspondences_return_no_more_without_a_draw():
    p = C.solver_problem(1, 19, 0.0, 0.0, True)
    S = R.Sim3Solver(p["X1"], p["X2"], p["sigma2_1"], p["sigma2_2"], p["K1"], p["K2"], True)
    out = S.iterate(5, np.zeros((0, 3), np.int32))
    assert out["no_more"] and not out["found"] and out["used"] == 0 and S.iterations == 0


def test_identical_sets_give_nan_and_no_pose():
    p = C.solver_problem(2, 40, 0.0, 0.0, True)
    S = R.Sim3Solver(p["X1"], p["X1"], p["sigma2_1"], p["sigma2_1"], p["K1"], p["K2"], True)
    out = S.find(C.draws(3, 40, S.max_its))
    assert not out["found"] and out["no_more"]
    assert S.best_inliers == 0 and S.iterations == S.max_its
    assert np.all(np.isnan(S.best_T12[:3]))


def test_thresholds_are_truncated_integers():
    _, sigma2 = C.orb_scales()
    e = R.max_errors(sigma2)
    assert e[0] == 9.0 and e[1] == 13.0  # 9.21, 9.21 * 1.44 = 13.26
    assert np.all(e == np.floor(9.210 * sigma2.astype(np.float64)))


def test_solver_finds_the_similarity_among_outliers():
    p = C.solver_problem(7, 120, 0.45, 0.5, False)
    S = R.Sim3Solver(p["X1"], p["X2"], p["sigma2_1"], p["sigma2_2"], p["K1"], p["K2"], False)
    out = S.find(C.draws(8, 120, S.max_its))
    assert out["found"] and out["n_inliers"] > 20
    assert np.all(p["truth"]["inliers"][out["mask"]])  # no gross outlier among the inliers
    assert abs(float(S.best_scale) - p["truth"]["s"]) < 0.05


# ------------------------------------------------------------------------------- SearchBySim3
SCALE, _ = C.orb_scales()


def run(kf1, kf2, sim3, matched=None, th=7.5):
    if matched is None:
        matched = np.full(len(kf1["skip"]), -1, np.int32)
    return R.search_by_sim3(kf1, kf2, sim3["s"], sim3["R"], sim3["t"], th, matched, C.K_KITTI,
                            C.W, C.H, SCALE)


@pytest.fixture(scope="module", params=[1.0, 1.15])
def base(request):
    kf1, kf2, sim3, pair = C.keyframe_pair(11, 120, s12=request.param)
    return kf1, kf2, sim3, pair, run(kf1, kf2, sim3)


def test_every_mutual_pair_is_recovered(base):
    kf1, kf2, sim3, pair, out = base
    nm = len(pair)
    assert np.array_equal(out["match"][:nm], pair)
    assert np.all(out["match"][nm:] == -1)
    assert out["n_found"] == nm
    assert np.array_equal(out["cand2"][pair], np.arange(nm))


def test_prior_matches_are_left_alone(base):
    kf1, kf2, sim3, pair, _ = base
    nm = len(pair)
    matched = np.full(len(kf1["skip"]), -1, np.int32)
    matched[0:10] = pair[0:10]   # matched to the point keyframe 2 holds at that key
    matched[10:20] = -2          # matched to points keyframe 2 does not hold
    out = run(kf1, kf2, sim3, matched)
    assert np.all(out["match"][:20] == -1) and np.all(out["cand1"][:20] == -1)
    assert np.all(out["cand2"][pair[0:10]] == -1)           # vbAlreadyMatched2
    assert np.array_equal(out["cand2"][pair[10:20]], np.arange(10, 20))  # still searched
    assert np.array_equal(out["match"][20:nm], pair[20:nm])
    assert out["n_found"] == nm - 20


def _only_change(a, b, i):
    d = np.flatnonzero(a != b)
    return list(d) == [i]


def test_each_skip_reason_removes_exactly_its_point(base):
    kf1, kf2, sim3, pair, ref = base
    i = 7
    k2 = int(pair[i])
    G2 = R.KeyFrameGrid(kf2["kps"], C.W, C.H)

    def variant(edit):
        a, b = C.copy_kf(kf1), C.copy_kf(kf2)
        edit(a, b)
        return run(a, b, sim3)

    def behind(a, b):
        a["Xw"][i] = C.world_point(a, C.into_camera1(sim3, [0.5, 0.2, -8.0]))

    def outside(a, b):
        a["Xw"][i] = C.world_point(a, C.into_camera1(sim3, [40.0, 0.0, 10.0]))

    def distance(a, b):
        a["max_dist"][i] = a["max_dist"][i] * f32(0.25)
        a["min_dist"][i] = a["min_dist"][i] * f32(0.25)

    def octave(a, b):
        b["kps"]["octave"][k2] = 0 if b["kps"]["octave"][k2] >= 3 else 7

    for name, edit in (("behind", behind), ("outside", outside), ("distance", distance),
                       ("octave", octave)):
        out = variant(edit)
        # wrong octave: nothing at the right level, or only a stranger above TH_HIGH
        assert out["reasons1"][i] in ((name, "far") if name == "octave" else (name,)), name
        assert _only_change(out["cand1"], ref["cand1"], i) and out["cand1"][i] == -1
        assert _only_change(out["match"], ref["match"], i)
        assert out["n_found"] == ref["n_found"] - 1

    # empty window: a point whose window in keyframe 2 holds its own key alone, the key moved away
    lone = None
    for j in range(len(pair)):
        kp = kf2["kps"][pair[j]]
        if len(G2.area(kp["x"], kp["y"], f32(7.5) * SCALE[kp["octave"] + 1])) == 1:
            lone = j
            break
    assert lone is not None

    def empty(a, b):
        q = b["kps"][pair[lone]]
        q["x"] = q["x"] + 200.0 if q["x"] < C.W / 2 else q["x"] - 200.0

    out = variant(empty)
    assert out["reasons1"][lone] == "empty"
    assert _only_change(out["cand1"], ref["cand1"], lone) and out["cand1"][lone] == -1
    assert out["n_found"] == ref["n_found"] - 1


def test_first_of_equal_distances_wins_and_disagreement_drops_the_pair(base):
    kf1, kf2, sim3, pair, ref = base
    rng = np.random.default_rng(3)
    G2 = R.KeyFrameGrid(kf2["kps"], C.W, C.H)
    done = 0
    for i in range(len(pair)):
        k2 = int(pair[i])
        kp = kf2["kps"][k2]
        if kp["octave"] < 3 or not 60 < kp["x"] < C.W - 60:
            continue
        d0 = int(R.hamming_rows(kf1["pdesc"][i], kf2["desc"][k2:k2 + 1])[0])
        for sign, winner_is_new in ((-1, True), (1, False)):
            b = C.copy_kf(kf2)
            n2 = len(b["skip"])
            new = np.zeros(1, C.KP_DTYPE)
            new[0] = kp
            new["x"] = kp["x"] + sign * 11.0
            cell_old = R.c_round(f32(kp["x"]) * G2.invW)
            cell_new = R.c_round(f32(new["x"][0]) * G2.invW)
            if cell_old == cell_new:
                continue
            # another descriptor at the same Hamming distance from the point's
            nd = np.unpackbits(kf1["pdesc"][i])
            nd[rng.choice(256, d0, replace=False)] ^= 1
            b["kps"] = np.concatenate([b["kps"], new])
            b["desc"] = np.concatenate([b["desc"], np.packbits(nd)[None]])
            for k in ("Xw", "min_dist", "max_dist", "pdesc"):
                b[k] = np.concatenate([b[k], b[k][:1]])
            b["skip"] = np.concatenate([b["skip"], np.ones(1, np.uint8)])
            out = run(kf1, b, sim3)
            if winner_is_new:  # the smaller cell column comes first in GetFeaturesInArea
                assert out["cand1"][i] == n2
                assert out["cand2"][k2] == i and out["match"][i] == -1  # the two disagree
                assert out["n_found"] == ref["n_found"] - 1
            else:
                assert out["cand1"][i] == k2 and out["match"][i] == k2
                assert out["n_found"] == ref["n_found"]
            done += 1
        if done >= 2:
            break
    assert done >= 2
