"""CPU tests that pin tests/voc_train_ref.py, the sequential restatement of DBoW2's create() the
GPU trainer is compared with (tests/test_gpu_voc_train.py), on cases worked by hand, and that the
C-ABI declares the training entry points."""
import os
import re

import numpy as np

import voc_train_ref as R
from conftest import ROOT


def _d(*bits):
    """A descriptor with these bits set (bit b: byte b // 8, mask 0x80 >> b % 8)."""
    d = np.zeros(32, np.uint8)
    for b in bits:
        d[b // 8] |= 0x80 >> (b % 8)
    return d


def test_header_declares_training_entry_points():
    src = open(os.path.join(ROOT, "include", "mmt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    syms = set(re.findall(r"\b(mmt_[a-z_0-9]+)\s*\(", src))
    assert {"mmt_train_vocabulary", "mmt_save_vocabulary"} <= syms


def test_majority_threshold():
    """FORB::meanValue sets a bit where count >= n / 2 + n % 2."""
    # 2 members differing in a bit: 1 >= 1 -> set
    assert np.array_equal(R.mean_value(np.stack([_d(5), _d()])), _d(5))
    # 3 members, 1 set: 1 < 2 -> clear; 2 set -> set
    assert np.array_equal(R.mean_value(np.stack([_d(5), _d(), _d()])), _d())
    assert np.array_equal(R.mean_value(np.stack([_d(5), _d(5, 9), _d()])), _d(5))
    # 4 members, 2 set: 2 >= 2 -> set
    assert np.array_equal(R.mean_value(np.stack([_d(5), _d(), _d(5), _d()])), _d(5))
    # a cluster of one member keeps that member
    assert np.array_equal(R.mean_value(np.stack([_d(1, 200)])), _d(1, 200))


def test_distance_and_first_of_equal_centres():
    assert list(R.distance(np.stack([_d(), _d(0, 255), _d(7)]), _d(7))) == [1, 3, 0]
    D = np.stack([_d(0), _d(1), _d(0, 1)])
    # both centres at distance 1 of every row: the first wins; equal centres: the first wins
    assert list(R.assign(D, [_d(0, 1, 2), _d(0, 1, 3)])) == [0, 0, 0]
    assert list(R.assign(D, [_d(1), _d(1)])) == [0, 0, 0]
    assert list(R.assign(D, [_d(0, 1, 2, 3), _d(1)])) == [1, 1, 1]


def test_prefix_sum_pick():
    md = [2, 3, 0, 5]
    assert R.pick_prefix(md, 5.0) == 1         # 2 + 3 >= 5 exactly
    assert R.pick_prefix(md, np.nextafter(5.0, 6.0)) == 3  # a zero distance is never picked
    assert R.pick_prefix(md, 1e-9) == 0
    assert R.pick_prefix(md, 10.0) == 3
    assert R.pick_prefix(md, 10.5) == 3        # past the end: the last feature


def test_random_stream_and_formulas():
    assert R.mix(0) == 0xE220A8397B1DCDAF      # splitmix64's first output from state 0
    assert R.draw(7, 0) == R.mix(7) >> 33 <= R.RAND_MAX
    assert R.child_key(5, 0) == R.mix(5 ^ 1) and R.child_key(5, 2) == R.mix(5 ^ 3)
    assert R.random_int(0, 10) == 0
    assert R.random_int(R.RAND_MAX, 10) == 9   # r / (RAND_MAX + 1.0) < 1
    assert R.random_int(1 << 30, 10) == 5
    assert R.random_int(1 << 30, 7) == 3
    assert R.random_value(R.RAND_MAX, 7) == 7.0
    assert R.random_value(0, 7) == 0.0
    assert R.random_value(1, R.RAND_MAX) == 1.0


def test_seeding_ends_early_without_k_distinct_descriptors():
    D = np.stack([_d(0), _d(1, 2), _d(3, 4, 5)] * 4)
    for seed in range(5):
        cl = R.seed_clusters(D, 5, R.mix(seed))
        assert len(cl) == 3
        assert sorted(int(R.POP8[c].sum()) for c in cl) == [1, 2, 3]
    assert len(R.seed_clusters(D, 2, R.mix(0))) == 2


def _octants():
    """8 features in a 2 x 2 x 2 hierarchy: the halves differ in 128 bits, the quarters in 64,
    the pairs in 8."""
    out = []
    for a in range(2):
        for b in range(2):
            for c in range(2):
                d = np.zeros(32, np.uint8)
                d[:16] = 255 * a
                d[16:24] = 255 * b
                d[24] = 255 * c
                out.append(d)
    return np.stack(out)


def test_id_order_is_hkmeansstep_s():
    """A node's children are contiguous, then each child's subtree in child order."""
    t = R.create([_octants()], 2, 3, seed=11)
    assert t.parent == [-1, 0, 0, 1, 1, 3, 3, 4, 4, 2, 2, 9, 9, 10, 10]
    assert t.words() == [5, 6, 7, 8, 11, 12, 13, 14]
    assert t.n_kmeans_nodes == 3 and t.n_capped == 0 and t.n_empty_clusters == 0
    # two levels: the quarters are words
    t = R.create([_octants()], 2, 2, seed=11)
    assert t.parent == [-1, 0, 0, 1, 1, 2, 2] and t.words() == [3, 4, 5, 6]
    # the trivial case: one child per feature, in feature order
    t = R.create([_octants()[:3]], 4, 2, seed=11)
    assert t.parent == [-1, 0, 0, 0]
    assert np.array_equal(np.stack(t.desc[1:]), _octants()[:3])


def test_idf_weights_and_unreached_word():
    A, B = _d(0), _d(100, 101)
    imgs = [np.stack([A, B]), np.stack([A])]  # a trivial root: words A, B and A's twin
    t = R.create(imgs, 3, 1, weighting=2)
    assert t.words() == [1, 2, 3]
    assert t.weight[1] == 0.0                    # in every image: log(2 / 2)
    assert t.weight[2] == float(np.log(2.0))     # in one of two images
    assert t.weight[3] == 0.0                    # the twin: duplicates go to the first
    t = R.create(imgs, 3, 1, weighting=1)        # TF: the idf part is 1
    assert [t.weight[w] for w in t.words()] == [1.0, 1.0, 1.0]


def test_iteration_cap_counts_nodes():
    rng = np.random.default_rng(3)
    D = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    t = R.create([D], 3, 1, max_iters=1)
    assert t.n_capped == 1 and t.iters == [1]
    t = R.create([D], 3, 1)
    assert t.n_capped == 0 and t.iters[0] >= 2


def test_saved_file_format_and_oracle_load(tmp_path, oracle_mod):
    rng = np.random.default_rng(4)
    imgs = [rng.integers(0, 256, (150, 32), dtype=np.uint8) for _ in range(4)]
    t = R.create(imgs, 4, 3, seed=2)
    p = str(tmp_path / "voc.txt")
    R.save_text(t, p)
    lines = open(p).read().split("\n")
    assert lines[0] == "4 3  0 0" and lines[-1] == ""
    assert re.fullmatch(r"\d+ [01] (\d+ ){32} \S+", lines[1])
    head, parent, leaf, desc, weight = R.read_text(p)
    assert list(parent) == t.parent[1:] and int(leaf.sum()) == len(t.words())
    ov = oracle_mod.Vocabulary(p)
    assert (ov.k, ov.L, ov.scoring, ov.weighting) == (4, 3, 0, 0)
    assert ov.n_nodes == t.n_nodes and ov.n_words == len(t.words())
    # the oracle's transform walks the tree to the same words
    D = np.concatenate(imgs)
    word_of = {n: i for i, n in enumerate(t.words())}
    mine = np.array([word_of[int(n)] for n in R.transform_words(t, D)], np.uint32)
    assert np.array_equal(ov.transform(D, 0)["word"], mine)
