"""GPU parity of SearchByBoW(KeyFrame*, KeyFrame*) for a batch of loop candidates
(mmt_search_by_bow_keyframes: k_bow_kf_nodes, k_bow_kf_nodes_wide, k_bow_kf_rot) against the
sequential restatement tests/bow_kf_ref_py.py: nmatches and every match12 entry bit for bit.

Shapes are the smallest at which each path can go wrong: the 64-lane chunk edges of the one-wave
kernel, its last node size (2048) and the wide kernel's first (2049), the wide kernel's
register-held positions (4096 / 4097), its largest node (16384), its 512-feature LDS tile of
keyframe 1 (511 / 512 / 513), and batches of 1, 2, 5 and 64 candidates.  Then the four steps of
LoopClosing::ComputeSim3 end to end against the chain of the restatements."""
import functools

import numpy as np
import pytest

import bow_kf_problems as KP
import bow_problems as BP
import bow_kf_ref_py as RK
import sim3_cases as C
import sim3_opt_cases as OC
import sim3_opt_ref_py as RO
import sim3_ref_py as R
from test_gpu_sim3_opt import _opt_problem, _solver_problem

pytestmark = pytest.mark.gpu
TOL = 1e-4  # the project's pose tolerance


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(nfeatures=2000))
    yield c
    c.close()


def check(ctx, kf1, cands, refs, ratio=0.75, orient=True):
    nm, m12 = ctx.search_by_bow_keyframes(kf1, cands, nnratio=ratio, check_orientation=orient)
    assert m12.shape == (len(cands), len(kf1[1]))
    for c, (nm_r, m_r) in enumerate(refs):
        print("candidate %d: nmatches gpu %d restatement %d" % (c, nm[c], nm_r))
        assert np.array_equal(m12[c], m_r), (c, np.nonzero(m12[c] != m_r)[0][:10])
        assert nm[c] == nm_r
    return nm, m12


# name: (keyframe-1 node sizes, candidate node sizes, generator options, ratio, orientation check)
SIZED = {
    "chunk_edges": ([2, 50, 50, 50], [1, 63, 64, 65], {}, 0.75, True),
    "narrow_last_2048": ([80], [2048], {}, 0.75, True),
    "wide_first_2049": ([80], [2049], {}, 0.75, True),
    "wide_registers_4096_4097": ([60, 60], [4096, 4097], {}, 0.75, True),
    "largest_node_16384": ([500], [16384], {}, 0.75, True),
    "lds_tile_511_512_513": ([511, 512, 513], [2100, 2100, 2100], {}, 0.75, True),
    "one_sided_nodes": ([40, 0, 40, 30, 0, 20], [0, 50, 60, 0, 0, 2060], {}, 0.75, True),
    "mp_valid1_0.3": ([80, 80], [300, 2200], {"mp_valid1": 0.3}, 0.75, True),
    "mp_valid2_0.3": ([80, 80], [300, 2200], {"mp_valid2": 0.3}, 0.75, True),
    "mp_valid2_none": ([80, 80], [300, 2200], {"mp_valid2": 0.0}, 0.75, True),
    "shuffled": ([30] * 20, [45] * 19 + [2070], {"shuffle": True}, 0.75, True),
    "no_orientation": ([30] * 20, [45] * 19 + [2070], {}, 0.75, False),
    "ratio_0.7": ([30] * 20, [45] * 19 + [2070], {"shuffle": True}, 0.7, True),
    "rotation_outliers_ties": ([30] * 120, [40] * 120, {"rot_outliers": 0.6, "dup": 0.3}, 0.75,
                               True),
}


@functools.lru_cache(maxsize=None)
def sized(name):
    """(keyframe 1, candidate, the restatement's (nmatches, match12)): computed once, shared."""
    s1, s2, kw, ratio, orient = SIZED[name]
    seed = 200 + sorted(SIZED).index(name)
    kf1, kf2 = KP.sized_problem(seed, s1, s2, **kw)
    return kf1, kf2, RK.search_by_bow_kf(kf1, kf2, ratio, orient)[:2]


@pytest.mark.parametrize("name", sorted(SIZED))
def test_matches_restatement(ctx, name):
    kf1, kf2, ref = sized(name)
    nm, _ = check(ctx, kf1, [kf2], [ref], SIZED[name][3], SIZED[name][4])
    if name == "mp_valid2_none":
        assert nm[0] == 0
    else:
        assert nm[0] > 10


def test_four_thousand_by_eight_thousand_keys(ctx):
    kf1, kf2 = KP.kf_problem(4, n_kf=4000, n_f=8000, n_nodes=120)
    ref = RK.search_by_bow_kf(kf1, kf2, 0.75, True)[:2]
    nm, _ = check(ctx, kf1, [kf2], [ref])
    assert nm[0] > 1000


@pytest.mark.parametrize("case,expect", [(KP.case_49_50, [0, -1]), (KP.case_no_mappoint, [1])])
def test_hand_built_cases(ctx, case, expect):
    kf1, kf2 = case()
    for orient in (False, True):
        nm_r, m_r, _ = RK.search_by_bow_kf(kf1, kf2, 0.75, orient)
        assert m_r.tolist() == expect
        check(ctx, kf1, [kf2], [(nm_r, m_r)], orient=orient)


# ------------------------------------------------------------------------------------- batches
@functools.lru_cache(maxsize=None)
def batch64():
    """One keyframe 1 and 64 candidates of six nodes each, with their restatement results."""
    kf1 = KP.keyframe1(50, [40, 30, 50, 20, 45, 35])
    sizes = [[50, 40, 70, 10, 64, 33], [0, 65, 20, 128, 1, 90], [130, 0, 63, 40, 0, 77]]
    cands = [KP.candidate(100 + c, kf1, sizes[c % 3], mp_valid=0.9 - 0.01 * (c % 7),
                          shuffle=c % 2 == 1) for c in range(64)]
    return kf1, cands, [RK.search_by_bow_kf(kf1, k)[:2] for k in cands]


@pytest.mark.parametrize("n_cand", [1, 2, 5, 64])
def test_batch_sizes(ctx, n_cand):
    kf1, cands, refs = batch64()
    nm, _ = check(ctx, kf1, cands[:n_cand], refs[:n_cand])
    assert (nm > 10).all()


EQUAL = {
    "1500x2000_120_nodes": lambda: KP.kf_problem(0),  # test_gpu_bow.py's first case, as keyframes
    "node_2048": lambda: sized("narrow_last_2048")[:2],
    "node_2049": lambda: sized("wide_first_2049")[:2],
    "node_4097": lambda: KP.sized_problem(90, [80], [4097]),
}


@functools.lru_cache(maxsize=None)
def equal_case(name):
    kf1, kf2 = EQUAL[name]()
    return kf1, kf2, RK.search_by_bow_kf(kf1, kf2)[:2]


@pytest.mark.parametrize("n_cand", [1, 8, 64])
@pytest.mark.parametrize("name", sorted(EQUAL))
def test_equal_candidates_share_a_launch(ctx, name, n_cand):
    """The same candidate n_cand times (each with its own copy in the staging block): every row is
    the restatement's.  These are the dispatches DESIGN §5l times."""
    kf1, kf2, ref = equal_case(name)
    check(ctx, kf1, [kf2] * n_cand, [ref] * n_cand)


def test_no_candidates_and_too_many(ctx):
    import multimot_track_amd as M
    kf1, cands, _ = batch64()
    nm, m12 = ctx.search_by_bow_keyframes(kf1, [])
    assert len(nm) == 0 and m12.shape == (0, len(kf1[1]))
    with pytest.raises(M.MmtError):
        ctx.search_by_bow_keyframes(kf1, cands + cands[:1])
    check(ctx, kf1, cands[:1], batch64()[2][:1])  # and the context still works


def test_mixed_batch_equals_single_calls(ctx):
    """Narrow-only candidates of different n, one with a wide node, one with an empty feature
    vector, one without keys: every row equals the candidate's single call and the restatement,
    and holds no index at or above its candidate's n."""
    kf1 = KP.keyframe1(60, [30, 60, 50, 20])
    narrow = KP.candidate(61, kf1, [100, 200, 0, 64])
    wide = KP.candidate(62, kf1, [50, 2100, 10, 0])
    small = KP.candidate(63, kf1, [5, 0, 9, 0])
    filled = KP.candidate(64, kf1, [20, 20, 20, 20])
    empty_fv = (KP.EMPTY_FV, filled[1], filled[2], filled[3])
    no_keys = (KP.EMPTY_FV, filled[1][:0], filled[2][:0], filled[3][:0])
    cands = [narrow, wide, empty_fv, no_keys, small, filled]
    refs = [RK.search_by_bow_kf(kf1, k)[:2] for k in cands]
    nm, m12 = check(ctx, kf1, cands, refs)
    assert nm[2] == 0 and nm[3] == 0 and (m12[2:4] == -1).all()
    assert nm[0] > 10 and nm[1] > 10
    for c, k in enumerate(cands):
        assert (m12[c] < len(k[1])).all()
        nm_1, m_1 = ctx.search_by_bow_keyframes(kf1, [k])
        assert nm_1[0] == nm[c] and np.array_equal(m_1[0], m12[c])


def test_keyframe1_without_keys_or_nodes(ctx):
    kf1, cands, _ = batch64()
    nm, m12 = ctx.search_by_bow_keyframes((KP.EMPTY_FV, kf1[1], kf1[2], kf1[3]), cands[:2])
    assert (nm == 0).all() and (m12 == -1).all() and m12.shape == (2, len(kf1[1]))
    nm, m12 = ctx.search_by_bow_keyframes((KP.EMPTY_FV, kf1[1][:0], kf1[2][:0], kf1[3][:0]),
                                          cands[:2])
    assert (nm == 0).all() and m12.shape == (2, 0)


# ------------------------------------------------------------------------------------ refusals
def _with_fv(kf, fv):
    return (fv, kf[1], kf[2], kf[3])


@pytest.mark.parametrize("side", [1, 2])
@pytest.mark.parametrize("what", ["unsorted", "out_of_range", "negative", "twice"])
def test_refusals(ctx, side, what):
    import multimot_track_amd as M
    kf1, cands, refs = batch64()
    kf = kf1 if side == 1 else cands[0]
    node, start, feat = kf[0]
    if what == "unsorted":
        bad = (node[::-1].copy(), start, feat)
    elif what == "out_of_range":
        bad = (node, start, np.where(np.arange(len(feat)) == 3, len(kf[1]), feat))
    elif what == "negative":
        bad = (node, start, np.where(np.arange(len(feat)) == 3, -1, feat))
    else:  # the last feature of the last node repeats the first of the first
        bad = (node, start, np.concatenate([feat[:-1], feat[:1]]))
    with pytest.raises(M.MmtError):
        if side == 1:
            ctx.search_by_bow_keyframes(_with_fv(kf, bad), cands[:2])
        else:
            ctx.search_by_bow_keyframes(kf1, [cands[1], _with_fv(kf, bad)])
    check(ctx, kf1, cands[:2], refs[:2])  # and the context still works


def test_node_of_16385_is_refused(ctx):
    import multimot_track_amd as M
    kf1 = KP.keyframe1(70, [10])
    kf2 = KP.candidate(71, kf1, [16385], frac_match=0.0)
    with pytest.raises(M.MmtError):
        ctx.search_by_bow_keyframes(kf1, [kf2])
    # keyframe 1's nodes have no such limit
    big1 = KP.keyframe1(72, [16385], mp_valid=0.01)
    kf2 = KP.candidate(73, big1, [40])
    check(ctx, big1, [kf2], [RK.search_by_bow_kf(big1, kf2)[:2]])


# -------------------------------------------------------------------- ComputeSim3, end to end
N_NODES = 40


def _bow_keyframe(kf, nodes):
    """A sim3_cases keyframe as SearchByBoW reads it: a key holds a MapPoint unless skipped."""
    return (BP.feature_vector(nodes), kf["kps"], kf["desc"], 1 - kf["skip"])


@functools.lru_cache(maxsize=None)
def loop_case():
    """A keyframe_pair of 220 common points (the true loop candidate) and, as the false one,
    keyframe 2 of an unrelated pair with the true candidate's first 8 keys copied in.  Vocabulary
    nodes are synthetic: a common point's two keys share a node, every other key's is random."""
    kf1, kf2, sim3, pair = C.keyframe_pair(31, 220, s12=1.1)
    _, other, _, _ = C.keyframe_pair(32, 220, s12=1.1)
    rng = np.random.default_rng(33)
    n1, n2 = len(kf1["skip"]), len(kf2["skip"])
    nodes1 = rng.integers(0, N_NODES, n1)
    nodes2 = rng.integers(0, N_NODES, n2)
    nodes2[pair] = nodes1[:len(pair)]
    nodes_other = rng.integers(0, N_NODES, len(other["skip"]))
    for name in ("kps", "desc", "Xw", "min_dist", "max_dist", "pdesc", "skip"):
        other[name][:8] = kf2[name][:8]
    nodes_other[:8] = nodes2[:8]
    return (kf1, kf2, other, sim3, _bow_keyframe(kf1, nodes1), _bow_keyframe(kf2, nodes2),
            _bow_keyframe(other, nodes_other))


def _compute_sim3(kf1, kf2, m12, solve, search, optimise):
    """LoopClosing::ComputeSim3 after SearchByBoW for one kept candidate (LoopClosing.cc:276-341),
    with every integer it decides on."""
    i1, sp = _solver_problem(kf1, kf2, m12)
    randi = C.draws(77, len(i1), 300)
    state, used, res = {}, 0, None
    for _ in range(60):
        res = solve(sp, randi[used:used + 5], state)
        used += 5
        if res["found"] or res["no_more"]:
            break
    ints = dict(n=len(i1), rounds=used // 5, found=bool(res["found"]),
                solver_inliers=int(res["n_inliers"]))
    if not res["found"]:
        return ints, None, None
    kept = np.full(len(m12), -1, np.int32)
    kept[i1[res["mask"]]] = m12[i1[res["mask"]]]
    s, Rm, t = state["best_scale"], state["best_R"], state["best_t"]
    new = search(kf1, kf2, s, Rm, t, kept)
    union = np.where(kept >= 0, kept, new)
    idx, op = _opt_problem(kf1, kf2, union, s, Rm, t)
    r = optimise(op)
    union[idx[~r["kept"]]] = -1
    ints.update(searched=int((new >= 0).sum()), n_edges=len(idx), n_inliers=int(r["n_inliers"]),
                accepted=bool(r["n_inliers"] >= 20))
    return ints, r, union


def test_compute_sim3_end_to_end(ctx):
    kf1, kf2, other, sim3, b1, b2, b_other = loop_case()
    scale, _ = C.orb_scales()
    nm_true, m_true, _ = RK.search_by_bow_kf(b1, b2, 0.75, True)
    nm_false, m_false, _ = RK.search_by_bow_kf(b1, b_other, 0.75, True)
    print("restatement: %d matches with the loop, %d with the other keyframe" % (nm_true, nm_false))
    assert nm_true >= 20 and 0 < nm_false < 20

    nm, m12 = check(ctx, b1, [b2, b_other], [(nm_true, m_true), (nm_false, m_false)])
    kept = [c for c in range(2) if nm[c] >= 20]  # LoopClosing.cc:264
    assert kept == [0]

    def ref_solve(sp, ri, st):
        if "S" not in st:
            st["S"] = R.Sim3Solver(sp["X1"], sp["X2"], sp["sigma2_1"], sp["sigma2_2"], sp["K1"],
                                   sp["K2"], sp["fix_scale"])
        o = st["S"].iterate(5, ri)
        st.update(best_scale=st["S"].best_scale, best_R=st["S"].best_R, best_t=st["S"].best_t)
        return o

    def ref_search(a, b, s, Rm, t, m):
        return R.search_by_sim3(a, b, s, Rm, t, 7.5, m, C.K_KITTI, C.W, C.H, scale)["match"]

    ri, ro, ru = _compute_sim3(kf1, kf2, m_true, ref_solve, ref_search, RO.optimize_sim3)
    gi, g, gu = _compute_sim3(
        kf1, kf2, m12[0],
        lambda sp, r5, st: ctx.sim3solver_iterate([sp], [r5], 5, [st])[0],
        lambda a, b, s, Rm, t, m: ctx.search_by_sim3(a, b, s, Rm, t, 7.5, m)[1],
        lambda op: ctx.optimize_sim3([op])[0])
    print("restatements:", ri)
    print("gpu:         ", gi)
    assert gi == ri
    assert gi["found"] and gi["accepted"] and gi["n_inliers"] >= 20
    assert np.array_equal(gu, ru)
    assert abs(float(g["s"]) - float(ro["s"])) <= TOL
    assert np.abs(np.asarray(g["R"], np.float64) - np.asarray(ro["R"], np.float64)).max() <= TOL
    assert np.abs(np.asarray(g["t"], np.float64) - np.asarray(ro["t"], np.float64)).max() <= TOL
    truth = dict(s=float(sim3["s"]), R=sim3["R"].astype(np.float64),
                 t=sim3["t"].astype(np.float64))
    print("error against the generating similarity: gpu %.3e restatements %.3e"
          % (OC.pose_error(g, truth), OC.pose_error(ro, truth)))
