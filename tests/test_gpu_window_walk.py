"""The boundaries of the cell walk that the projection matchers share (wave_window_walk under
k_fuse_cand, k_sim3_search, k_local_cand, k_sbp_frame and k_match_fix's rescan), which the fixture
frames reach only by chance: a window over all 64 grid columns, a window of one cell, windows of
exactly 64, 65 and 128 keys (the ends of the 64-position passes) where position alone decides the
winner, an empty cell range, non-finite projections, and rescans past the kCandK kept candidates.
Expected values are the CPU oracle's and tests/sim3_ref_py.py's, bit for bit; every test first
checks, on the reference side, that its inputs reach the condition it is about."""
import numpy as np
import pytest

import sim3_cases as SC
import sim3_ref_py as R
import window_cases as WC

pytestmark = pytest.mark.gpu
BF = 387.5744
EYE = np.eye(4, dtype=np.float32)
TH = 3.0                  # Fuse and SearchBySim3: radius th * scale[level]
TH_LOCAL = 1.2            # SearchLocalPoints at viewCos 1: radius 2.5 * th * scale[level]
R0 = np.float32(3.0)      # both at level 0
TH_ALL, TH_LOCAL_ALL = 1300.0, 600.0  # radii above the image width


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(nfeatures=2000))
    yield c
    c.close()


@pytest.fixture(scope="module")
def scale(ctx, oracle_mod):
    s, _ = SC.orb_scales()
    assert np.array_equal(np.asarray(ctx.levels()["scale"], np.float32)[:len(s)], s)
    assert np.array_equal(np.asarray(oracle_mod.orb_config()["scale"], np.float32), s)
    return s


def grid(oracle_mod, kf):
    _, _, cs, ci = oracle_mod.frame_stereo_grid(kf["kps"], kf["depth"], SC.K_KITTI, BF)
    return cs, ci


def all_three(ctx, oracle_mod, scale, kf, th, th_local):
    """The keyframe's three points through Fuse, SearchBySim3 and SearchLocalPoints against their
    references; returns the references' answers (fuse key per point, sim3 key per point,
    local match per key)."""
    P = kf["points"]
    a = (kf["kps"], kf["desc"], kf["depth"], EYE, P["Xw"], P["normal"], P["min_dist"],
         P["max_dist"], P["pdesc"])
    io, do = oracle_mod.fuse_candidates(*a, SC.K_KITTI, BF, SC.W, SC.H, th=th)
    ig, dg = ctx.fuse_candidates(*a, th=th)
    print("fuse", io, do, ig, dg)
    assert np.array_equal(ig, io) and np.array_equal(dg, do)
    kf1, kf2, s = WC.sim3_pair(kf)
    none = np.full(len(kf1["skip"]), -1, np.int32)
    ref = R.search_by_sim3(kf1, kf2, s["s"], s["R"], s["t"], th, none, SC.K_KITTI, SC.W, SC.H,
                           scale)
    nf, match, c1, c2 = ctx.search_by_sim3(kf1, kf2, s["s"], s["R"], s["t"], th, none)
    print("sim3", ref["cand1"], c1)
    assert np.array_equal(c1, ref["cand1"]) and np.array_equal(c2, ref["cand2"])
    assert np.array_equal(match, ref["match"]) and nf == ref["n_found"]
    b = a + (np.zeros(len(P["min_dist"]), np.uint8), th_local)
    onm, omatch, ofrus = oracle_mod.search_local_points(*b, SC.K_KITTI, BF, scale)
    nm, lmatch, frus = ctx.search_local_points(*b)
    print("local", onm, np.nonzero(omatch >= 0)[0], nm, np.nonzero(lmatch >= 0)[0])
    assert np.array_equal(frus, ofrus) and np.all(ofrus[:, 0] == 1) and np.all(ofrus[:, 1] == 2)
    assert nm == onm and np.array_equal(lmatch, omatch)
    return io, ref["cand1"], omatch


@pytest.mark.parametrize("winner", ["first", "last"])
@pytest.mark.parametrize("n_pile", [64, 65, 128])
def test_pass_boundaries_one_cell_and_empty_range(ctx, oracle_mod, scale, n_pile, winner):
    kf = WC.walk_keyframe(n_pile, winner)
    cs, ci = grid(oracle_mod, kf)
    r = WC.radius(R0)
    # the pile's window walks exactly n_pile keys, all of them the pile's, from two cells
    pile = WC.keys_in_range(cs, ci, WC.cell_range(*WC.PILE_UV, r))
    assert len(pile) == n_pile and sorted(pile) == list(range(n_pile))
    assert {WC.cell_of(*kf["kps"][["x", "y"]][k]) for k in pile} == \
        {(WC.PILE_COL - 1, WC.PILE_ROW), (WC.PILE_COL, WC.PILE_ROW)}
    want = pile[0] if winner == "first" else pile[-1]
    assert want != 0 and np.all(kf["desc"][pile] == kf["D"])
    assert [k for k in pile if kf["kps"]["octave"][k] == WC.LEVEL] == \
        (pile if winner == "first" else [want])
    # the empty point's cells hold no key; the corner point's window is the grid's last cell
    assert WC.keys_in_range(cs, ci, WC.cell_range(*WC.EMPTY_UV, r)) == []
    assert WC.cell_range(*WC.CORNER_UV, r) == (63, 63, 47, 47)
    corner = WC.keys_in_range(cs, ci, (63, 63, 47, 47))
    assert corner == [n_pile, n_pile + 1]
    fuse, sim3, local = all_three(ctx, oracle_mod, scale, kf, TH, TH_LOCAL)
    # what the references answered: the first key in GetFeaturesInArea order wins its ties
    assert list(fuse) == [want, -1, corner[0]] and list(sim3) == [want, -1, corner[0]]
    assert local[want] == 0 and local[corner[0]] == 2 and (local >= 0).sum() == 2


def test_window_over_every_column(ctx, oracle_mod, scale):
    kf = WC.walk_keyframe(128, "first", n_background=167)
    n = len(kf["kps"])
    cs, ci = grid(oracle_mod, kf)
    for r0 in (TH_ALL, 2.5 * TH_LOCAL_ALL):
        assert WC.radius(r0) > SC.W
        for uv in (WC.PILE_UV, WC.EMPTY_UV, WC.CORNER_UV):
            rng4 = WC.cell_range(*uv, WC.radius(r0))
            assert rng4 == (0, 63, 0, 47) and len(WC.keys_in_range(cs, ci, rng4)) == n == 300
    fuse, sim3, local = all_three(ctx, oracle_mod, scale, kf, TH_ALL, TH_LOCAL_ALL)
    # without Fuse's reprojection gate the twin in column 2 is the first of the equal distances
    first = WC.keys_in_range(cs, ci, (0, 63, 0, 47))
    twin = next(k for k in first if np.all(kf["desc"][k] == kf["D"]))
    assert WC.cell_of(*kf["kps"][["x", "y"]][twin]) == WC.TWIN_CELLS[0]
    assert list(sim3) == [twin] * 3 and fuse[0] != twin and fuse[0] >= 0


def test_non_finite_projections(ctx, oracle_mod, scale):
    kf = WC.walk_keyframe(64, "first")
    P = kf["points"]
    bad = np.array([[np.nan] * 3, [np.inf, 0.5, 10.0], [0.5, 0.2, np.inf], [np.nan, 0.2, 9.0]],
                   np.float32)
    Xw = np.concatenate([P["Xw"][:1], bad, P["Xw"][2:]])
    m = len(Xw)
    pick = [0] + [0] * len(bad) + [2]
    # SearchLocalPoints: a NaN point fails none of isInFrustum's tests (all negated comparisons)
    a = (kf["kps"], kf["desc"], kf["depth"], EYE, Xw, P["normal"][pick], P["min_dist"][pick],
         P["max_dist"][pick], P["pdesc"][pick], np.zeros(m, np.uint8), TH_LOCAL)
    onm, omatch, ofrus = oracle_mod.search_local_points(*a, SC.K_KITTI, BF, scale)
    assert ofrus[1, 0] == 1 and np.isnan(ofrus[1, 2]) and onm == 2
    nm, match, frus = ctx.search_local_points(*a)
    print("local", onm, ofrus, nm, frus)
    assert np.array_equal(frus, ofrus, equal_nan=True)
    assert nm == onm and np.array_equal(match, omatch)
    # SearchByProjection(Frame, Frame): active last-frame points with NaN and inf coordinates
    lk = np.zeros(m, kf["kps"].dtype)
    lk["x"], lk["y"], lk["octave"], lk["size"] = 50.0 + 20.0 * np.arange(m), 200.0, WC.LEVEL, 31.0
    b = (kf["kps"], kf["desc"], kf["depth"], EYE, lk, Xw, P["pdesc"][pick],
         np.ones(m, np.uint8), EYE, 7.0)
    onm, omatch = oracle_mod.search_by_projection_frame(*b, SC.K_KITTI, BF, scale, False, True)
    assert onm == 2 and sorted(omatch[omatch >= 0]) == [0, m - 1]
    nm, match = ctx.search_by_projection_frame(*b, mono=False, check_orientation=True)
    print("sbp", onm, np.nonzero(omatch >= 0)[0], nm, np.nonzero(match >= 0)[0])
    assert nm == onm and np.array_equal(match, omatch)


def test_rescan_past_the_kept_candidates(ctx, oracle_mod, scale):
    c = WC.rescan_case()
    cs, ci = grid(oracle_mod, c)
    nk, cp = c["n_keys"], c["copies"]
    assert cp > 8 and nk > cp  # more copies than kCandK, and a key left for the last one
    fx, fy, cx, cy = SC.K_KITTI
    for j in range(0, len(c["Xw"]), cp):  # every point's window holds its own n_keys keys
        X = c["Xw"][j]
        uv = (fx * X[0] / X[2] + cx, fy * X[1] / X[2] + cy)
        keys = WC.keys_in_range(cs, ci, WC.cell_range(*uv, WC.radius(R0)))
        assert sorted(keys) == list(range(j // cp * nk, (j // cp + 1) * nk))
    a = (c["kps"], c["desc"], c["depth"], EYE, c["Xw"], c["normal"], c["min_dist"],
         c["max_dist"], c["pdesc"], np.zeros(len(c["Xw"]), np.uint8), TH_LOCAL)
    onm, omatch, ofrus = oracle_mod.search_local_points(*a, SC.K_KITTI, BF, scale)
    # every copy binds a key of its own: copies 9 to 12 went past the first eight candidates
    assert onm == len(c["Xw"]) and sorted(omatch[omatch >= 0]) == list(range(len(c["Xw"])))
    nm, match, frus = ctx.search_local_points(*a)
    print("rescan", onm, omatch, nm, match)
    assert np.array_equal(frus, ofrus)
    assert nm == onm and np.array_equal(match, omatch)
