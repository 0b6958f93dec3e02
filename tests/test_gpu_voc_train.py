"""GPU tests of vocabulary training (mmt_train_vocabulary, mmt_save_vocabulary; mmt_voctrain.hip)
against tests/voc_train_ref.py, the sequential restatement of DBoW2's create().

Every decision of create() is an integer (Hamming distances, vote counts, prefix sums of integer
distances), so the level-batched GPU trainer must produce the depth-first restatement's tree byte
for byte: parents, leaf flags, descriptors, word order and the Lloyd iteration counts; the weights
(a double log on either side) must agree in the six digits saveToTextFile prints.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import voc_train_ref as R
from conftest import GOLDEN, load_kitti_frame

pytestmark = pytest.mark.gpu

VOC = os.path.join(GOLDEN, "test_voc_k10l6.txt")
BOW_KEYS = ("bow_frames", "trk", "trk_ok", "reloc", "reloc_ok", "reloc_cands", "pnp_found",
            "sbp_rounds", "triangulated", "sft_matches", "kfdb")


def _split(D, n_images):
    return [np.ascontiguousarray(a) for a in np.array_split(D, n_images)]


def _clustered(rng, n, n_centres, flip):
    c = rng.integers(0, 256, (n_centres, 32), dtype=np.uint8)
    noise = np.packbits(rng.random((n, 256)) < flip, axis=1)
    return c[rng.integers(0, n_centres, n)] ^ noise


def _few_bits(rng, n, bits):
    """Descriptors over a handful of bits: few distinct values, so equal distances and exact
    majority ties occur at every level."""
    D = np.zeros((n, 32), np.uint8)
    on = rng.random((n, len(bits))) < 0.5
    for j, b in enumerate(bits):
        D[on[:, j], b // 8] |= 0x80 >> (b % 8)
    return D


@functools.lru_cache(maxsize=None)
def _kitti_descs():
    import multimot_track_amd as M
    from oracle import oracle as O
    ctx = M.Context(M.kitti03_config(1242, 375, 2000))
    try:
        return tuple(ctx.orb_extract(O.gray_from_bgr(load_kitti_frame(i)["bgr"]))[1]
                     for i in range(5))
    finally:
        ctx.close()


def _inputs(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "trivial_root":        # N = 7 <= k: one child per feature
        return _split(rng.integers(0, 256, (7, 32), dtype=np.uint8), 2), 10, 3
    if name == "n_is_k_plus_1":       # the smallest node that runs k-means
        return _split(rng.integers(0, 256, (11, 32), dtype=np.uint8), 3), 10, 3
    if name == "k2":
        return _split(_clustered(rng, 500, 12, 0.08), 4), 2, 4
    if name == "k20":
        return _split(_clustered(rng, 2500, 40, 0.08), 5), 20, 2
    if name == "L1":
        return _split(_clustered(rng, 1000, 9, 0.1), 4), 5, 1
    if name == "L10_ragged":          # the recursion ends long before level 10
        return _split(_clustered(rng, 200, 6, 0.1), 3), 2, 10
    if name == "four_distinct":       # seeding ends at dist_sum == 0, identical leaves
        base = rng.integers(0, 256, (4, 32), dtype=np.uint8)
        return _split(base[rng.integers(0, 4, 1200)], 6), 10, 3
    if name == "few_bits":
        return _split(_few_bits(rng, 1500, (3, 40, 41, 100, 200, 255)), 5), 3, 6
    if name == "items_20000":         # nodes of several work items, hundreds of nodes per level
        return _split(_clustered(rng, 20011, 60, 0.12), 20), 3, 5
    if name == "kitti":
        return list(_kitti_descs()), 10, 6
    raise KeyError(name)


CASES = ("trivial_root", "n_is_k_plus_1", "k2", "k20", "L1", "L10_ragged", "four_distinct",
         "few_bits", "items_20000", "kitti")


@functools.lru_cache(maxsize=None)
def _reference(name, weighting=0, scoring=0, seed=0):
    imgs, k, L = _inputs(name)
    return R.create(imgs, k, L, weighting, scoring, seed)


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(1242, 375, 2000))
    yield c
    c.close()


def _compare(ctx, tmp_path, name, weighting=0, scoring=0, seed=0):
    imgs, k, L = _inputs(name)
    t = _reference(name, weighting, scoring, seed)
    st = ctx.train_vocabulary(imgs, k, L, weighting, scoring, seed)
    pg, pr = str(tmp_path / "gpu.txt"), str(tmp_path / "ref.txt")
    ctx.save_vocabulary(pg)
    R.save_text(t, pr)
    hg, parent_g, leaf_g, desc_g, w_g = R.read_text(pg)
    hr, parent_r, leaf_r, desc_r, w_r = R.read_text(pr)
    print(name, "nodes", st["n_nodes"], "words", st["n_words"], "iters", st["iters"], "ref",
          t.iters, "kmeans nodes", st["n_kmeans_nodes"], "empty", st["n_empty_clusters"])
    assert hg == hr
    assert np.array_equal(parent_g, parent_r)
    assert np.array_equal(leaf_g, leaf_r)
    assert np.array_equal(desc_g, desc_r)
    assert w_g == w_r
    assert st["iters"] == t.iters
    assert st["n_capped"] == 0 and t.n_capped == 0
    assert (st["n_nodes"], st["n_words"], st["n_kmeans_nodes"], st["n_empty_clusters"]) == \
        (t.n_nodes, len(t.words()), t.n_kmeans_nodes, t.n_empty_clusters)
    return st, t


@pytest.mark.parametrize("name", CASES)
def test_tree_equals_restatement(ctx, tmp_path, name):
    _compare(ctx, tmp_path, name)


@pytest.mark.parametrize("weighting,scoring", [(0, 1), (1, 0), (2, 0), (3, 1)])
def test_weightings(ctx, tmp_path, weighting, scoring):
    """TF_IDF is the default of every other case; here the others, and the L2 scoring."""
    _compare(ctx, tmp_path, "k2", weighting, scoring)


def test_other_seed_other_tree_same_seed_same_bytes(ctx, tmp_path):
    imgs, k, L = _inputs("k20")
    out = []
    for i, seed in enumerate((5, 5, 6)):
        ctx.train_vocabulary(imgs, k, L, seed=seed)
        p = str(tmp_path / ("v%d.txt" % i))
        ctx.save_vocabulary(p)
        out.append(open(p, "rb").read())
    assert out[0] == out[1]
    assert out[0] != out[2]
    _compare(ctx, tmp_path, "k20", seed=6)


def test_iteration_cap(ctx, tmp_path):
    """max_iters = 1: every k-means node stops after its first assignment and is counted."""
    imgs, k, L = _inputs("L1")
    st = ctx.train_vocabulary(imgs, k, L, max_iters=1)
    t = R.create(imgs, k, L, max_iters=1)
    assert st["iters"] == t.iters == [1]
    assert st["n_capped"] == t.n_capped == 1
    p = str(tmp_path / "cap.txt")
    ctx.save_vocabulary(p)
    R.save_text(t, str(tmp_path / "ref.txt"))
    assert open(p).read() == open(str(tmp_path / "ref.txt")).read()


def test_saved_file_round_trip_and_oracle_transform(ctx, tmp_path, oracle_mod):
    """train -> save -> load_vocabulary -> bow_transform equals the oracle's transform of the saved
    file bit for bit, and walks to the words and nodes of the in-memory tree."""
    imgs = list(_kitti_descs())
    D = np.concatenate(imgs)
    ctx.train_vocabulary(imgs, 10, 6)
    w0, x0, n0 = ctx.bow_transform(D, 4)
    p = str(tmp_path / "voc.txt")
    ctx.save_vocabulary(p)
    ctx.load_vocabulary(p)
    ov = oracle_mod.Vocabulary(p)
    for levelsup in (4, 2):
        w, x, nd = ctx.bow_transform(D, levelsup)
        r = ov.transform(D, levelsup)
        assert np.array_equal(w, r["word"])
        assert np.array_equal(x, r["weight"])
        assert np.array_equal(nd, r["node"])
    w, x, nd = ctx.bow_transform(D, 4)
    assert np.array_equal(w, w0) and np.array_equal(nd, n0)
    assert np.allclose(x, x0, rtol=1e-5, atol=0)  # six printed digits against full precision
    # the saved file saved again is the same file
    p2 = str(tmp_path / "voc2.txt")
    ctx.save_vocabulary(p2)
    assert open(p).read() == open(p2).read()


def test_golden_vocabulary_save_load_same_transform(ctx, tmp_path):
    D = np.concatenate(list(_kitti_descs()))
    ctx.load_vocabulary(VOC)
    a = ctx.bow_transform(D, 4)
    p = str(tmp_path / "golden_again.txt")
    ctx.save_vocabulary(p)
    ctx.load_vocabulary(p)
    b = ctx.bow_transform(D, 4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert np.allclose(a[1], b[1], rtol=1e-5, atol=0)


def test_refusals(tmp_path):
    import multimot_track_amd as M
    rng = np.random.default_rng(9)
    imgs = _split(rng.integers(0, 256, (60, 32), dtype=np.uint8), 3)
    c = M.Context(M.kitti03_config(1242, 375, 2000))
    try:
        with pytest.raises(M.MmtError, match="-22"):
            c.save_vocabulary(str(tmp_path / "none.txt"))      # nothing to save yet
        for kw in (dict(k=1), dict(k=21), dict(L=0), dict(L=11), dict(scoring=2)):
            args = dict(k=4, L=2)
            args.update(kw)
            with pytest.raises(M.MmtError, match="-22"):
                c.train_vocabulary(imgs, **args)
        with pytest.raises(M.MmtError, match="-22"):
            c.train_vocabulary([], 4, 2)                         # no images
        with pytest.raises(M.MmtError, match="-22"):
            c.train_vocabulary([np.zeros((0, 32), np.uint8)] * 2, 4, 2)  # no descriptors
        # a non-monotone image_start, through the C-ABI
        D = np.concatenate(imgs)
        start = np.array([0, 40, 20, 60], np.int32)
        prm = M.MmtVocTrainParams(4, 2, 0, 0, 0, 0)
        st = M.MmtVocTrainStats()
        rc = M.lib().mmt_train_vocabulary(c.handle, D.ctypes.data, start.ctypes.data, 3,
                                          ctypes.byref(prm), ctypes.byref(st))
        assert rc == -22
        with pytest.raises(M.MmtError, match="-22"):
            c.save_vocabulary(str(tmp_path / "none.txt"))      # a refused call installs nothing
        c.train_vocabulary(imgs, 4, 2)
        with pytest.raises(M.MmtError, match="-22"):
            c.save_vocabulary(str(tmp_path / "no_such_dir" / "v.txt"))
        # MMT_ESTATE once the map has a keyframe, as mmt_load_vocabulary
        f = load_kitti_frame(0)
        c.track(f["bgr"], f["disp"], f["flow"], f["sem"])
        with pytest.raises(M.MmtError, match="-77"):
            c.train_vocabulary(imgs, 4, 2)
        c.save_vocabulary(str(tmp_path / "still.txt"))          # saving stays allowed
    finally:
        c.close()


def _drive_pair(oracle_mod, voc, W, H, K, bf, nfeat, n, lost, chunk=16):
    """test_gpu_vocab.py's drive with this vocabulary file on both sides."""
    import torch
    import multimot_track_amd as M
    from multimot_track_amd import scene
    Rr = scene.SequenceRenderer(scene.StreetScene(3, 1003), W, H, K=K, device=torch.device("cuda:0"))
    seq = Rr.sequence(n)
    for i in lost:
        seq["bgr"][i] = 128
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
    finally:
        c.close()
    tr = oracle_mod.Tracker(W, H, (K["fx"], K["fy"], K["cx"], K["cy"]), bf, 0, nfeat)
    tr.set_vocabulary(voc)
    ora = []
    for i in range(n):
        f = scene.to_numpy_frames({k: seq[k][i:i + 1] for k in ("bgr", "disp", "flow", "mask")})[0]
        ora.append(tr.track(f["bgr"], f["disp"], f["flow"], f["sem"]))
    return got, ora, gb, tr.bow_stats()


def test_trained_vocabulary_tracking_matches_oracle(oracle_mod, tmp_path):
    """End to end: a k = 4, L = 6 vocabulary trained on the ORB descriptors of synthetic street
    frames (other scenes than the drive's), saved, and loaded by the tracker and by the oracle for
    the 3/4-resolution 40-frame drive with a textureless frame: parity record clean, vocabulary
    counters equal."""
    import torch
    import multimot_track_amd as M
    from multimot_track_amd import scene
    from oracle import compare
    W, H, nfeat = 931, 281, 1000
    K = {k: v * 0.75 for k, v in scene.KITTI03.items()}
    cfg = M.kitti03_config(W, H, nfeat)
    cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.bf = K["fx"], K["fy"], K["cx"], K["cy"], K["bf"]
    c = M.Context(cfg)
    p = str(tmp_path / "trained_k4l6.txt")
    try:
        imgs = []
        for seed in (2311, 2312):
            Rr = scene.SequenceRenderer(scene.StreetScene(3, seed), W, H, K=K,
                                        device=torch.device("cuda:0"))
            seq = Rr.sequence(20)
            for i in range(0, 20, 5):
                f = scene.to_numpy_frames({k: seq[k][i:i + 1]
                                           for k in ("bgr", "disp", "flow", "mask")})[0]
                imgs.append(c.orb_extract(oracle_mod.gray_from_bgr(f["bgr"]))[1])
        st = c.train_vocabulary(imgs, 4, 6, seed=2313)
        assert st["n_capped"] == 0 and st["n_words"] > 500
        c.save_vocabulary(p)
    finally:
        c.close()
    got, ora, gb, ob = _drive_pair(oracle_mod, p, W, H, K, K["bf"], nfeat, 40, [24])
    rec = compare.parity_record(got, ora)
    print("trained", st, "\nparity", rec, "\nbow counters", gb)
    assert rec["first_divergent_frame"] is None, rec
    assert {k: gb[k] for k in BOW_KEYS} == {k: ob[k] for k in BOW_KEYS}, (gb, ob)
    assert gb["bow_frames"] > 0
