"""GPU parity of the two matchers of the vocabulary path against the CPU oracle, through the C-ABI
probes that call the tracking path's own code: mmt_search_by_projection_keyframe (k_sbp_kf and
its host replay, Relocalization's SearchByProjection(F, KF, sAlreadyFound, th, ORBdist)) and
mmt_search_for_triangulation (the query build, k_sft and the per-pair collection of
CreateNewMapPoints).  Every binding, count and F12 is compared bit for bit on the cases of
reloc_problems; test_oracle_reloc_match.py pins the oracle side of the same cases to a Python
restatement of the reference and asserts each case's property."""
import ctypes

import numpy as np
import pytest

import match_problems as MP
import reloc_problems as RP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(RP.W, RP.H, 2000))
    yield c
    c.close()


@pytest.fixture(scope="module")
def scale(oracle_mod):
    return MP.scale_factors(oracle_mod)


@pytest.mark.parametrize("name", RP.SBP_CASES)
def test_search_by_projection_keyframe_matches_oracle(ctx, oracle_mod, scale, name):
    c = RP.sbp_case(oracle_mod, name)
    nm_o, m_o = oracle_mod.search_by_projection_keyframe(*RP.sbp_args(c), RP.K, RP.BF, scale)
    nm_g, m_g, n_rescan = ctx.search_by_projection_keyframe(*RP.sbp_args(c))
    print("%s: nmatches %d (oracle %d), n_rescan %d" % (name, nm_g, nm_o, n_rescan))
    assert np.array_equal(m_g, m_o), (np.nonzero(m_g != m_o)[0][:10], m_g[m_g != m_o][:10],
                                       m_o[m_g != m_o][:10])
    assert nm_g == nm_o
    if name.startswith("crowded"):
        # later copies of the point find all 32 listed keys bound: the host rescan binds them
        assert n_rescan > 0
        assert nm_o == len(c["tags"]["copies"])


@pytest.mark.parametrize("name", RP.SFT_CASES)
def test_search_for_triangulation_matches_oracle(ctx, oracle_mod, scale, name):
    c = RP.sft_case(oracle_mod, name)
    nm_o, m_o, F_o = oracle_mod.search_for_triangulation(c["kf1"], c["kf2s"], RP.K, RP.BF, scale)
    nm_g, m_g, F_g = ctx.search_for_triangulation(c["kf1"], c["kf2s"])
    print("%s: nmatches %s (oracle %s)" % (name, nm_g.tolist(), nm_o.tolist()))
    assert np.array_equal(F_g.view(np.uint32), F_o.view(np.uint32)), (F_g, F_o)
    assert np.array_equal(m_g, m_o), (np.argwhere(m_g != m_o)[:10], m_g[m_g != m_o][:10],
                                       m_o[m_g != m_o][:10])
    assert np.array_equal(nm_g, nm_o)


def test_search_for_triangulation_no_pairs(ctx, oracle_mod):
    c = RP.sft_case(oracle_mod, "ties")
    nm, m, F = ctx.search_for_triangulation(c["kf1"], [])
    assert len(nm) == 0 and m.shape == (0, len(c["kf1"]["kps"])) and len(F) == 0


def test_probes_reject_bad_arguments(ctx, oracle_mod):
    import multimot_track_amd as M
    L = M.lib()
    EINVAL = -22  # MMT_EINVAL
    # SearchForTriangulation: a feature listed in two nodes, in keyframe 1 and in a neighbour
    c = RP.sft_case(oracle_mod, "ties")
    node, start, feat = c["kf2s"][0]["fv"]
    twice = dict(c["kf2s"][0], fv=(node, start, np.concatenate([feat[:-1], feat[:1]])))
    with pytest.raises(M.MmtError):
        ctx.search_for_triangulation(c["kf1"], [twice])
    with pytest.raises(M.MmtError):
        ctx.search_for_triangulation(twice, c["kf2s"])
    unsorted = dict(c["kf2s"][0], fv=(node[::-1].copy(), start, feat))
    with pytest.raises(M.MmtError):
        ctx.search_for_triangulation(c["kf1"], [unsorted])
    # null arrays with n > 0, and n_pairs < 0
    keep = []
    a = M._sft_keyframe(c["kf1"], keep)
    b = M._sft_keyframe(c["kf2s"][0], keep)
    m12 = np.zeros(a.n, np.int32)
    F = np.zeros(9, np.float32)
    nm = np.zeros(1, np.int32)

    def sft(a, npairs, b):
        return L.mmt_search_for_triangulation(ctx.handle, ctypes.addressof(a), npairs,
                                              ctypes.addressof(b), M._p(m12), M._p(F), M._p(nm))
    assert sft(a, 1, b) == 0
    assert sft(a, -1, b) == EINVAL
    for field in ("kps", "desc", "uR", "has_mp"):
        for which in (0, 1):
            bad_a = M._sft_keyframe(c["kf1"], keep)
            bad_b = M._sft_keyframe(c["kf2s"][0], keep)
            setattr((bad_a, bad_b)[which], field, None)
            assert sft(bad_a, 1, bad_b) == EINVAL, (field, which)
    assert L.mmt_search_for_triangulation(ctx.handle, ctypes.addressof(a), 1, None, M._p(m12),
                                          M._p(F), M._p(nm)) == EINVAL
    assert L.mmt_search_for_triangulation(ctx.handle, ctypes.addressof(a), 1,
                                          ctypes.addressof(b), None, M._p(F), M._p(nm)) == EINVAL
    # SearchByProjection(F, KF): null arrays with m > 0 or n > 0
    s = RP.sbp_case(oracle_mod, "m5")
    assert ctx.search_by_projection_keyframe(*RP.sbp_args(s))[0] == 5
    keep = []
    fr = ctx._match_frame(s["kps"], s["desc"], s["depth"], s["tcw"], keep)
    arrs = [np.ascontiguousarray(s[k], np.float32) for k in ("Xw", "min_dist", "max_dist", "angle")]
    match = np.zeros(fr.n, np.int32)
    nmo, nr = ctypes.c_int(0), ctypes.c_int(0)

    def sbp(P, skip=s["skip"], bound=s["bound"], out=match, frame=fr):
        return L.mmt_search_by_projection_keyframe(
            ctx.handle, ctypes.byref(frame), ctypes.byref(P),
            None if skip is None else skip.ctypes.data, 10.0, 100,
            None if bound is None else bound.ctypes.data, None if out is None else M._p(out),
            ctypes.byref(nmo), ctypes.byref(nr))

    def points(**over):
        P = M.MmtKeyFramePoints()
        P.m = 5
        P.Xw, P.min_dist, P.max_dist, P.angle = [x.ctypes.data for x in arrs]
        P.desc = s["pdesc"].ctypes.data
        for k, v in over.items():
            setattr(P, k, v)
        return P
    assert sbp(points()) == 0 and nmo.value == 5
    for field in ("Xw", "min_dist", "max_dist", "desc", "angle"):
        assert sbp(points(**{field: None})) == EINVAL, field
    assert sbp(points(m=-1)) == EINVAL
    assert sbp(points(), skip=None) == EINVAL
    assert sbp(points(), bound=None) == EINVAL
    assert sbp(points(), out=None) == EINVAL
    nodesc = ctx._match_frame(s["kps"], None, s["depth"], s["tcw"], keep)
    assert sbp(points(), frame=nodesc) == EINVAL


def test_search_by_projection_keyframe_nothing_listed(ctx, oracle_mod):
    """No point (m = 0) and eight points all skipped: nothing is uploaded or launched, every key
    stays unbound and no point reaches the host rescan."""
    c = RP.sbp_case(oracle_mod, "m5")
    args = list(RP.sbp_args(c))
    n = len(c["kps"])
    for m in (0, 8):
        args[4] = np.resize(c["Xw"], (m, 3))
        args[5], args[6] = np.resize(c["min_dist"], m), np.resize(c["max_dist"], m)
        args[7], args[8] = np.resize(c["pdesc"], (m, 32)), np.resize(c["angle"], m)
        args[9] = np.ones(m, np.uint8)
        nm, match, n_rescan = ctx.search_by_projection_keyframe(*args)
        assert nm == 0 and n_rescan == 0 and len(match) == n and np.all(match == -1), m


def test_search_for_triangulation_empty_keyframe1(ctx, oracle_mod):
    """No pair, and one pair against a keyframe 1 without keys: OK, no query, no match."""
    c = RP.sft_case(oracle_mod, "ties")
    empty = dict(kps=np.zeros(0, RP.KP), desc=np.zeros((0, 32), np.uint8),
                 uR=np.zeros(0, np.float32), has_mp=np.zeros(0, np.uint8),
                 fv=(np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.int32)),
                 Tcw=c["kf1"]["Tcw"])
    nm, m, F = ctx.search_for_triangulation(empty, [])
    assert len(nm) == 0 and m.shape == (0, 0)
    nm, m, F = ctx.search_for_triangulation(empty, c["kf2s"][:1])
    assert nm.tolist() == [0] and m.shape == (1, 0) and F.shape == (1, 3, 3)
