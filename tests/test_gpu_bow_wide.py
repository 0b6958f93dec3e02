"""GPU parity of SearchByBoW (C4) over wide vocabulary nodes: a frame node of more than 2048
features goes to the workgroup-wide kernel k_bow_nodes_wide (mmt_match.hip), up to the matchers'
16384-key cap.  Probe cases against the CPU oracle (every binding and nmatches bit-exact): the
first size over the one-wave limit, sizes one past a multiple of the workgroup, the C5 size, two
wide nodes with shuffled lists, the cap itself, mostly invalid MapPoints, nothing matching, and
wide and narrow nodes in one call.  Then the tracker with a two-level vocabulary (depth <= 4:
DBoW2 files every feature of a frame under node 0) at 4000 features against the oracle, frame by
frame, through TrackReferenceKeyFrame, Relocalization and CreateNewMapPoints."""
import numpy as np
import pytest

import bow_problems as BP

pytestmark = pytest.mark.gpu

BOW_KEYS = ("bow_frames", "trk", "trk_ok", "reloc", "reloc_ok", "reloc_cands", "pnp_found",
            "sbp_rounds", "triangulated", "sft_matches", "kfdb")


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(nfeatures=2000))
    yield c
    c.close()


def _per_feature_node(fv, n):
    node, start, feat = fv
    out = np.zeros(n, np.int64)
    for k in range(len(node)):
        out[feat[start[k]:start[k + 1]]] = node[k]
    return out


def _mixed_problem():
    """Case D: 40 nodes, those below 20 merged into node 0 (one wide frame node beside twenty
    narrow ones), the lists of both vectors reshuffled."""
    pr = list(BP.bow_problem(23, n_nodes=40, n_kf=3000, n_f=6000, rot_outliers=0.5, dup=0.3))
    for slot, n in ((0, 3000), (4, 6000)):
        nodes = _per_feature_node(pr[slot], n)
        nodes[nodes < 20] = 0
        pr[slot] = BP.feature_vector(nodes, np.random.default_rng(30))
    sizes = np.diff(pr[4][1])
    assert len(sizes) == 21 and sizes.max() == 2983 and np.sort(sizes)[-2] <= 2048
    assert sizes.min() >= 124
    return tuple(pr)


_PROBLEMS = {}


def _problem(name, seed, kw):
    """Each problem is built once and shared by its (ratio, orientation) cases."""
    if name not in _PROBLEMS:
        _PROBLEMS[name] = _mixed_problem() if name == "D" else BP.bow_problem(seed, **kw)
    return _PROBLEMS[name]


@pytest.mark.parametrize("name,seed,kw,ratio,orient,nm_ref", [
    ("A", 20, {"n_nodes": 1, "n_kf": 1500, "n_f": 2049}, 0.7, True, 594),
    ("A", 20, {"n_nodes": 1, "n_kf": 1500, "n_f": 2049}, 0.75, False, 734),
    ("E", 24, {"n_nodes": 1, "n_kf": 300, "n_f": 2112, "frac_match": 0.1}, 0.7, True, 98),
    ("F", 25, {"n_nodes": 1, "n_kf": 600, "n_f": 4097}, 0.7, True, 295),
    ("B", 21, {"n_nodes": 1, "n_kf": 4000, "n_f": 8000}, 0.7, True, 1853),
    ("C", 22, {"n_nodes": 2, "n_kf": 6000, "n_f": 16000, "shuffle": True}, 0.75, False, 3303),
    ("G", 26, {"n_nodes": 1, "n_kf": 500, "n_f": 16384}, 0.7, True, 233),
    ("H", 27, {"n_nodes": 1, "n_kf": 2500, "n_f": 3000, "mp_valid": 0.3}, 0.75, False, 380),
    ("I", 28, {"n_nodes": 1, "n_kf": 400, "n_f": 2600, "frac_match": 0.0}, 0.7, True, 0),
    ("D", 23, None, 0.7, True, 747),
    ("D", 23, None, 0.75, False, 1187),
])
def test_search_by_bow_wide_matches_oracle(ctx, oracle_mod, name, seed, kw, ratio, orient, nm_ref):
    pr = _problem(name, seed, kw)
    assert np.diff(pr[4][1]).max() > 2048  # a wide frame node
    nm_o, m_o = oracle_mod.search_by_bow(*pr, nnratio=ratio, check_orientation=orient)
    assert nm_o == nm_ref  # the reference alone: the problem is the one the case names
    nm_g, m_g = ctx.search_by_bow(*pr, nnratio=ratio, check_orientation=orient)
    assert nm_g == nm_o
    assert np.array_equal(m_g, m_o), np.nonzero(m_g != m_o)[0][:10]
    if name != "I":
        assert nm_o > 20


def test_search_by_bow_rejects_node_over_cap(ctx):
    """One frame node of 16385 features: refused by the host's argument check."""
    import multimot_track_amd as M
    pr = BP.bow_problem(29, n_nodes=1, n_kf=50, n_f=16385, frac_match=0.0)
    assert np.diff(pr[4][1]).max() == 16385
    with pytest.raises(M.MmtError):
        ctx.search_by_bow(*pr)


def _write_shallow_vocabulary(path):
    """A k = 10, L = 2 vocabulary in DBoW2's text format: ten inner nodes under the root, ten
    words under each."""
    rng = np.random.default_rng(3)

    def desc():
        return " ".join(str(int(v)) for v in rng.integers(0, 256, 32))

    lines = ["0 0 %s 0" % desc() for _ in range(10)]
    for p in range(10):
        for _ in range(10):
            d = desc()  # the bytes before the weight
            lines.append("%d 1 %s %.17g" % (p + 1, d, rng.uniform(0.2, 2.0)))
    with open(path, "w") as f:
        f.write("10 2 0 0\n" + "\n".join(lines))


def test_shallow_vocabulary_tracking_matches_oracle(oracle_mod, tmp_path):
    """1242x375 at 4000 features with a two-level vocabulary: every frame's BoW feature vector is
    the single node 0 with all ~4000 keys.  The GPU tracker takes the oracle's path frame by frame
    (one textureless frame: TrackReferenceKeyFrame, Relocalization, CreateNewMapPoints), with equal
    vocabulary counters and the same final map."""
    import torch
    import multimot_track_amd as M
    from map_invariants import same_map
    from multimot_track_amd import scene
    from oracle import compare
    voc = str(tmp_path / "voc_k10l2.txt")
    _write_shallow_vocabulary(voc)
    W, H, nfeat, n, chunk, bf = 1242, 375, 4000, 26, 13, 387.5744
    K = dict(scene.KITTI03)
    R = scene.SequenceRenderer(scene.StreetScene(3, 1003), W, H, K=K,
                               device=torch.device("cuda:0"))
    seq = R.sequence(n)
    seq["bgr"][18] = 128
    cfg = M.kitti03_config(W, H, nfeat, max_batch=chunk)
    cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.bf = K["fx"], K["fy"], K["cx"], K["cy"], bf
    c = M.Context(cfg)
    got = []
    try:
        c.load_vocabulary(voc)
        for s0 in range(0, n, chunk):
            sl = slice(s0, min(n, s0 + chunk))
            got += c.track_chunk_device(seq["bgr"][sl], seq["disp"][sl], seq["flow"][sl],
                                        seq["mask"][sl])
        gb = c.bow_counters()
        gm = c.map_dump()
    finally:
        c.close()
    tr = oracle_mod.Tracker(W, H, (K["fx"], K["fy"], K["cx"], K["cy"]), bf, 0, nfeat)
    tr.set_vocabulary(voc)
    ora = []
    for i in range(n):
        f = scene.to_numpy_frames({k: seq[k][i:i + 1] for k in ("bgr", "disp", "flow", "mask")})[0]
        ora.append(tr.track(f["bgr"], f["disp"], f["flow"], f["sem"]))
    ob, om = tr.bow_stats(), tr.map_dump()
    # the oracle alone: the wide-node path is taken
    assert ora[1]["n_keys"] > 2048
    assert ob["trk"] >= 2 and ob["trk_ok"] >= 1 and ob["reloc_ok"] >= 1
    assert ob["triangulated"] > 100
    rec = compare.parity_record(got, ora)
    assert rec["first_divergent_frame"] is None, rec
    assert {k: gb[k] for k in BOW_KEYS} == {k: ob[k] for k in BOW_KEYS}, (gb, ob)
    diff, fmax = same_map(gm, om)
    assert diff == [] and fmax < 1e-3, (diff, fmax)
    assert np.abs(gm["kf_T"] - om["kf_T"]).max() < 1e-4
