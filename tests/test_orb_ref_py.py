"""CPU tests of the NumPy restatement of ORB extraction (tests/orb_ref_py.py) and, through it, of
the C++ oracle (oracle/orb_ref.cpp):

* known answers of the restatement itself, worked by hand below from the definitions;
* oracle against restatement, stage by stage and exact, on the inputs the GPU tests build on;
* the comparison helpers report a difference when the restatement's inputs are perturbed, so an
  equal result above is not an artefact of a helper that cannot fail.
"""
import functools
import hashlib
import math

import numpy as np
import pytest

import orb_ref_py as R
from multimot_track_amd import synthetic

F = np.float32

# SHA-256 of bit_pattern_31_ (reference src/ORBextractor.cc:150-407) as 1024 little-endian int32.
# Computed once from the reference's source when this test was written (the initialiser parsed as
# decimal integers, comments stripped); a recorded result, no reference text.  It pins
# csrc/orb_pattern.inc, which the kernels, the oracle and the restatement all read.
PATTERN_SHA256 = "7e645581387b82784797e8adddb9b6f0c12611859fda09ca8a9bec96d767a05f"


def test_pattern_digest():
    pat = R.load_pattern()
    assert pat.shape == (512, 2)
    assert hashlib.sha256(pat.astype("<i4").tobytes()).hexdigest() == PATTERN_SHA256
    assert np.abs(pat).max() <= 13  # every rotated test stays inside the 31-px patch


# ------------------------------------------------------------------ known answers: FAST
def _ring(center, values):
    """7x7 patch: `center` everywhere, circle pixel k (Appendix A.5 order) set to values[k]."""
    p = np.full((7, 7), center, np.uint8)
    for (dx, dy), v in zip(R.CIRCLE, values):
        p[3 + dy, 3 + dx] = v
    return p


def test_fast_arc_known_answers():
    # exactly 9 contiguous brighter pixels (k = 2..10), the weakest brighter by 25: a corner for
    # every threshold below 25, so cornerScore = 24
    vals = [100] * 16
    for k, b in zip(range(2, 11), (30, 33, 25, 40, 31, 29, 50, 26, 35)):
        vals[k] = 100 + b
    assert R.fast_cell(_ring(100, vals), 20).tolist() == [[3.0, 3.0, 24.0]]
    # the threshold is strict: p > v + t
    assert R.fast_cell(_ring(100, vals), 24).tolist() == [[3.0, 3.0, 24.0]]
    assert len(R.fast_cell(_ring(100, vals), 25)) == 0
    # one pixel fewer: an 8-arc is no corner at any threshold
    vals8 = list(vals)
    vals8[10] = 100
    assert len(R.fast_cell(_ring(100, vals8), 20)) == 0
    assert len(R.fast_cell(_ring(100, vals8), 1)) == 0
    # a darker arc that wraps from k = 12 round to k = 4, weakest darker by 22 -> score 21; the
    # other pixels brighter by 10 change nothing
    vals = [110] * 16
    for k in (12, 13, 14, 15, 0, 1, 2, 3, 4):
        vals[k] = 100 - 22 - k
    assert R.fast_cell(_ring(100, vals), 20).tolist() == [[3.0, 3.0, 21.0]]
    # an arc of 10 with its weakest pixel at one end: the best 9-arc drops it.  d = 30 x 9, then 21
    vals = [100] * 16
    for k in range(5, 14):
        vals[k] = 130
    vals[14] = 121
    assert R.fast_cell(_ring(100, vals), 20).tolist() == [[3.0, 3.0, 29.0]]
    # an isolated pixel brighter by c: all 16 circle pixels darker by c -> score c - 1
    img = np.full((9, 9), 50, np.uint8)
    img[4, 5] = 50 + 64
    assert R.fast_cell(img, 20).tolist() == [[5.0, 4.0, 63.0]]
    # images with fewer than 7 rows or columns have no detection region
    assert len(R.fast_cell(np.zeros((6, 30), np.uint8), 20)) == 0


def test_nms_ties_known_answers():
    z = np.zeros((5, 6), np.int32)
    s = z.copy()
    s[2, 2] = s[2, 3] = 50               # equal neighbours: strict '>' keeps neither
    assert len(R.nms(s)) == 0
    s[2, 3] = 49
    assert R.nms(s).tolist() == [[2.0, 2.0, 50.0]]
    s = z.copy()
    s[1, 1] = s[2, 2] = 40               # diagonal neighbours tie as well
    assert len(R.nms(s)) == 0
    s = z.copy()
    s[0, 0], s[4, 5], s[2, 2], s[2, 4] = 9, 8, 30, 30   # scores outside the region are 0
    assert R.nms(s).tolist() == [[0.0, 0.0, 9.0], [2.0, 2.0, 30.0], [4.0, 2.0, 30.0],
                                 [5.0, 4.0, 8.0]]  # row-major; two apart is no neighbour


def test_cell_loop_min_threshold_known_answer():
    # 100 x 100 level: width = height = 100 - 32 = 68 -> 2 x 2 cells of 34, cell (i, j) starting
    # at 16 + 34 * (i, j) and 40 px wide; detection regions tile [19, 81) without overlap.
    cells = R.level_cells(100, 100)
    assert [(c[2], c[3], c[4], c[5]) for c in cells] == [(16, 56, 16, 56), (16, 56, 50, 84),
                                                         (50, 84, 16, 56), (50, 84, 50, 84)]
    img = np.full((100, 100), 100, np.uint8)
    img[30, 30] = 130   # cell (0, 0): fires at iniTh 20 with score 29
    img[40, 40] = 110   # same cell, contrast 10: below iniTh, and the cell is not retried
    img[30, 70] = 110   # cell (0, 1): only fires at minTh 7, score 9
    img[70, 30] = 106   # cell (1, 0): contrast 6 fires at neither threshold
    img[52, 75] = 125   # row 52 is cell row 0's last detection row (16 + 40 - 4); cell (0, 1)
    got = R.level_candidates(img, 20, 7)
    # keys are relative to the minBorder corner (16, 16), cells in row-major order; in cell (0, 1)
    # the iniTh pass finds (75, 52) alone, so the contrast-10 dot at (70, 30) is not reported
    assert got.tolist() == [[14.0, 14.0, 29.0], [59.0, 36.0, 24.0]]
    img[52, 75] = 100
    assert R.level_candidates(img, 20, 7).tolist() == [[14.0, 14.0, 29.0], [54.0, 14.0, 9.0]]


def test_cell_loop_equals_fast_per_cell():
    """level_candidates cuts cells from one score map per threshold; the reference calls FAST on
    every cell's submatrix.  Both must give the same list."""
    img = synthetic.gray_frame(131, 187, 3)
    want = []
    for (i, j, r0, r1, c0, c1, wc, hc) in R.level_cells(187, 131):
        k = R.fast_cell(img[r0:r1, c0:c1], 20)
        if len(k) == 0:
            k = R.fast_cell(img[r0:r1, c0:c1], 7)
        k[:, 0] += j * wc
        k[:, 1] += i * hc
        want.append(k)
    want = np.concatenate(want)
    assert len(want) > 50
    R.check_key_list("cell loop", R.level_candidates(img, 20, 7), want)


# ------------------------------------------------------------------ known answers: octree
_OCT = dict(A=(10, 10, 5), B=(20, 20, 9), C=(60, 10, 7), D=(90, 40, 3), E=(10, 60, 4),
            F=(40, 90, 8), G=(60, 60, 6), H=(90, 90, 6), I=(70, 70, 2), J=(30, 30, 9))


def _oct(names):
    return [list(map(float, _OCT[n])) for n in names]


def test_distribute_known_answers():
    # Region 100 x 100: nIni = round(100 / 100) = 1.  First pass splits the root at (50, 50):
    #   n1 = {A, B, J}, n2 = {C, D}, n3 = {E, F}, n4 = {G, H, I}; pushed to the front in that
    #   order, so the list reads n4, n3, n2, n1 (4 nodes).
    cands = np.array(_oct("ABCDEFGHIJ"), F)
    # quota 1 and 2: 4 nodes >= N ends the loop.  Best of each node, first wins ties:
    #   n4: G (6) before H (6); n3: F; n2: C; n1: B (9) before J (9).
    for N in (1, 2, 4):
        assert R.distribute(cands, 0, 100, 0, 100, N).tolist() == _oct("GFCB")
    # quota 5: 4 < 5 and 4 + 3 * 4 > 5 -> the sorted pass.  Sizes (3, 2, 2, 3) for n1..n4; sorted
    #   ascending by (size, creation) and walked from the back: n4 first.  n4 splits at (75, 75)
    #   into {G, I} and {H}; the list reads {H}, {G, I}, n3, n2, n1 = 5 nodes -> stop.
    assert R.distribute(cands, 0, 100, 0, 100, 5).tolist() == _oct("HGFCB")
    # quota 6: next in the walk is n1 (size 3, created before n4): splits at (25, 25) into
    #   {A, B} and {J}; the list reads {J}, {A, B}, {H}, {G, I}, n3, n2.
    assert R.distribute(cands, 0, 100, 0, 100, 6).tolist() == _oct("JBHGFC")
    # a quota nothing can reach: every key ends in a node of its own (all 10 kept)
    got = R.distribute(cands, 0, 100, 0, 100, 50)
    assert sorted(got.tolist()) == sorted(_oct("ABCDEFGHIJ"))
    # two initial nodes: round(200 / 100) = 2, hX = 100; keys go to node int(x / hX)
    assert R.n_ini(0, 200, 0, 100) == 2 and R.n_ini(0, 149, 0, 100) == 1
    assert R.n_ini(0, 150, 0, 100) == 2  # C round(): half away from zero
    two = np.array([[10, 10, 1], [30, 30, 2], [150, 50, 3]], F)
    # node 0 = {(10,10), (30,30)}, node 1 = {(150,50)} (one key: never split).  Quota 1: the pass
    # splits node 0 at (50, 50): both keys in its n1 -> list {n1}, node 1 = 2 nodes >= 1.
    assert R.distribute(two, 0, 200, 0, 100, 1).tolist() == [[30.0, 30.0, 2.0],
                                                             [150.0, 50.0, 3.0]]
    assert len(R.distribute(np.zeros((0, 3), F), 0, 200, 0, 100, 5)) == 0


# ------------------------------------------------------------------ known answers: angle, BRIEF
def test_ic_angle_half_planes():
    umax = R.config()["umax"]
    assert umax == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    yy, xx = np.indices((41, 41))
    for mask, want in ((xx > 20, 0.0), (yy > 20, 90.0), (xx < 20, 180.0), (yy < 20, 270.0)):
        img = np.where(mask, 200, 10).astype(np.uint8)
        m01, m10 = R.ic_moments(img, [20.0], [20.0], umax)
        assert (m01[0] == 0) != (m10[0] == 0)  # the moment along the edge vanishes by symmetry
        assert R.ic_angle(img, [20.0], [20.0], umax).tolist() == [want]
    # moments by the definition, on a random patch: sums of u * I and v * I over the disc
    img = np.random.default_rng(1).integers(0, 256, (41, 41)).astype(np.uint8)
    m01 = m10 = 0
    for v in range(-15, 16):
        for u in range(-umax[abs(v)], umax[abs(v)] + 1):
            m10 += u * int(img[20 + v, 20 + u])
            m01 += v * int(img[20 + v, 20 + u])
    assert [int(a[0]) for a in R.ic_moments(img, [20.0], [20.0], umax)] == [m01, m10]


def test_fast_atan2_known_answers():
    assert R.fast_atan2(0, 0) == 0 and R.fast_atan2(0, 5) == 0
    assert R.fast_atan2(5, 0) == 90 and R.fast_atan2(0, -5) == 180 and R.fast_atan2(-5, 0) == 270
    # the diagonal: c = 1 / (1 + eps) = 1 in float32, so the angle is the float32 sum p7 + p5 + p3
    # + p1 in Horner order, about 44.992 (the polynomial's known error at 45 degrees)
    rad = F(180.0 / math.pi)
    p = [F(c) * rad for c in (0.9997878412794807, -0.3258083974640975, 0.1555786518463281,
                              -0.04432655554792128)]
    want = ((p[3] + p[2]) + p[1]) + p[0]
    assert R.fast_atan2(3, 3) == want and abs(float(want) - 45) < 0.02
    assert R.fast_atan2(3, -3) == F(180) - want and R.fast_atan2(-3, -3) == F(360) - (F(180) - want)
    ys, xs = np.mgrid[-20:21, -20:21]
    ref = np.degrees(np.arctan2(ys, xs)) % 360
    assert np.abs(R.fast_atan2(ys, xs).astype(np.float64) - ref).max() < 0.02


def test_descriptor_of_two_valued_patch():
    pat = R.load_pattern()
    x0, y0, x1, y1 = (pat[0::2, 0], pat[0::2, 1], pat[1::2, 0], pat[1::2, 1])
    yy, xx = np.indices((41, 41))
    img = np.where(xx > 20, 200, 50).astype(np.uint8)  # bright where x > 0 about the key
    # angle 0: a = 1, b = 0, the tests are unrotated -> bit q = (x0 <= 0 < x1)
    d = R.descriptors(img, [20.0], [20.0], [0.0], pat)
    want = np.packbits((x0 <= 0) & (x1 > 0), bitorder="little")
    assert d.shape == (1, 32) and d[0].tolist() == want.tolist()
    assert 0 < int(np.unpackbits(d).sum()) < 256
    # angle 90: b = 1 and a = (float)cos(pi/2 as float) = -4.37e-8, which a test coordinate of
    # at most 13 cannot carry across a rounding boundary: column = -y, row = x -> bit q = (y0 >= 0
    # > y1)
    assert F(math.cos(float(F(90) * F(math.pi / 180.0)))) == F(-4.371138828673793e-08)
    d = R.descriptors(img, [20.0], [20.0], [90.0], pat)
    want = np.packbits((y0 >= 0) & (y1 < 0), bitorder="little")
    assert d[0].tolist() == want.tolist()
    # byte i holds tests 8i .. 8i + 7, test 8i in bit 0 (ORBextractor.cc:123-143)
    first = [(x0[q] <= 0) and (x1[q] > 0) for q in range(8)]
    d = R.descriptors(img, [20.0], [20.0], [0.0], pat)
    assert d[0, 0] == sum(int(b) << q for q, b in enumerate(first))


def test_blur_and_resize_known_answers():
    img = np.zeros((21, 21), np.uint8)
    img[10, 10] = 255
    taps = np.array(R.GAUSS_TAPS, np.int64)
    assert taps.sum() == 256
    assert (R.blur7(img)[7:14, 7:14] == (np.outer(taps, taps) * 255 + 32768) >> 16).all()
    # REFLECT_101 at a corner: pixel (0, 0) sees taps folded about index 0 (the edge pixel once)
    img = np.zeros((21, 21), np.uint8)
    img[0, 0] = 255
    fold = np.array([56, 48 * 2, 34 * 2, 18 * 2], np.int64)  # weight of source index 0..3 at x = 0
    assert R.blur7(img)[0, 0] == (56 * 56 * 255 + 32768) >> 16
    img[:] = 0
    img[1, 2] = 255
    assert R.blur7(img)[0, 0] == (fold[1] * fold[2] * 255 + 32768) >> 16
    # resize by exactly 1/2: fx = 0.5 everywhere -> coefficients (1024, 1024), the mean of a 2 x 2
    # block rounded half up: (a + b + c + d + 2) >> 2 in Q22 arithmetic
    src = np.random.default_rng(2).integers(0, 256, (8, 12)).astype(np.uint8)
    s = src.astype(np.int64)
    want = (1024 * (1024 * (s[0::2, 0::2] + s[0::2, 1::2]) + 1024 * (s[1::2, 0::2] + s[1::2, 1::2]))
            + (1 << 21)) >> 22
    assert (R.resize_level(src, 6, 4) == want).all()
    # 1242 -> 1035 (level 1 of a KITTI frame): scale 1.2; dx = 0 reads fx = 0.1 -> (1843, 205),
    # the last column dx = 1034 has fx = (1034.5 * 1.2 - 0.5) - 1240 = 0.9 -> (205, 1843)
    row = np.zeros((1, 1242), np.uint8)
    row[0, 0], row[0, 1], row[0, 1240], row[0, 1241] = 200, 100, 40, 240
    out = R.resize_level(np.repeat(row, 2, 0), 1035, 2)
    assert out[0, 0] == (2048 * (200 * 1843 + 100 * 205) + (1 << 21)) >> 22
    assert out[0, 1034] == (2048 * (40 * 205 + 240 * 1843) + (1 << 21)) >> 22


def test_config_known_answers():
    assert R.config(2000)["n_per_level"] == [434, 362, 302, 251, 209, 175, 145, 122]
    assert R.level_sizes(1242, 375) == [(1242, 375), (1035, 312), (862, 260), (719, 217),
                                        (599, 181), (499, 151), (416, 126), (347, 105)]


def test_fast_tile_geometry_bound():
    """The widest FAST cell any level can have is 59 px (one cell column on a level of width - 32
    in [30, 59]; two or more columns give at most ceil(89 / 2) + 6 = 51), so the LDS tile width
    ((cols + 4) & ~3) never exceeds 60: tests/test_gpu_orb_stages.py uses a 59-px cell as the
    limit of k_fast<72>."""
    worst = 0
    for lw in range(62, 1300):
        worst = max(worst, max(c[5] - c[4] for c in R.level_cells(lw, 62)))
    assert worst == 59 and ((worst + 4) & ~3) == 60


def test_gpu_shape_table_entries_are_the_smallest():
    """tests/test_gpu_orb_stages.py asserts why each shape is in its table; here, without a GPU,
    that no narrower (or, for the blur band, lower) accepted image meets the same condition."""
    import test_gpu_orb_stages as T
    for name, (w, h, why) in T.SHAPES.items():
        assert T._accepted(w, h) and why(w, h), name
        if name == "400x260":
            continue  # kept for continuity with the older tests, not as a smallest shape
        if name == "blur_h1":
            assert not any(why(w, hh) for hh in range(T.HMIN, h)), name
        else:
            first = 1229 if w > 700 else T.WMIN
            assert not any(why(ww, h) for ww in range(first, w)), name
    assert (T.WMIN, T.HMIN) == SMALLEST


# ------------------------------------------------------------------ oracle against restatement
def _edge_images():
    """The noise, low_contrast and checker images of test_gpu_orb.test_orb_edge_cases."""
    h, w = 480, 640
    rng = np.random.default_rng(9)
    noise = rng.integers(0, 256, (h, w), dtype=np.uint8)
    low = (120 + rng.integers(0, 12, (h, w))).astype(np.uint8)
    checker = ((np.indices((h, w)).sum(0) // 5) % 2 * 200 + 20).astype(np.uint8)
    return dict(noise=noise, low_contrast=low, checker=checker)


SMALLEST = (221, 221)  # smallest accepted image, asserted in test_smallest_accepted_size

INPUTS = ("kitti0", "synth400x260", "smallest", "low_contrast", "checker", "noise")


@functools.lru_cache(maxsize=None)
def _input(name):
    """(gray, nfeatures) of a named input; images are read-only from here on."""
    if name == "kitti0":
        from conftest import load_kitti_frame
        from oracle import oracle as O
        g, nf = O.gray_from_bgr(load_kitti_frame(0)["bgr"]), 2000
    elif name == "synth400x260":
        g, nf = synthetic.gray_frame(260, 400, 6), 300
    elif name == "smallest":
        g, nf = synthetic.gray_frame(SMALLEST[1], SMALLEST[0], 7), 300
    else:
        g, nf = np.ascontiguousarray(_edge_images()[name][:240, :320]), 1000
    g.setflags(write=False)
    return g, nf


@functools.lru_cache(maxsize=None)
def _stages(name):
    g, nf = _input(name)
    return R.orb_stages(g, nf)


def test_smallest_accepted_size():
    # a level needs at least one 30-px FAST cell row and column: size - 32 >= 30 at level 7
    w, h = SMALLEST
    assert R.level_sizes(w, h)[7] == (62, 62)
    assert R.level_sizes(w - 1, h)[7][0] == 61 and R.level_sizes(w, h - 1)[7][1] == 61
    assert len(R.level_cells(62, 62)) == 1


@pytest.mark.parametrize("name", INPUTS)
def test_oracle_pyramid_and_blur(name, oracle_mod):
    g, _ = _input(name)
    st = _stages(name)
    pyr = oracle_mod.pyramid(g)
    R.check_images(name + " pyramid", pyr, st["pyramid"])
    R.check_images(name + " blur", [oracle_mod.blur7(p) for p in pyr], st["blur"])
    assert oracle_mod.level_sizes(g.shape[1], g.shape[0])[0].tolist() == \
        [p.shape[1] for p in st["pyramid"]]


@pytest.mark.parametrize("name", INPUTS)
def test_oracle_candidates_and_distribute(name, oracle_mod):
    g, nf = _input(name)
    st = _stages(name)
    assert list(oracle_mod.orb_config(nf)["n_per_level"]) == st["cfg"]["n_per_level"]
    total = 0
    for l, img in enumerate(st["pyramid"]):
        cand = oracle_mod.level_candidates(img)
        R.check_key_list("%s level %d candidates" % (name, l), cand, st["cands"][l])
        h, w = img.shape
        N = st["cfg"]["n_per_level"][l]
        sel = oracle_mod.distribute(cand, 16, w - 16, 16, h - 16, N)
        mine = R.distribute(st["cands"][l], 16, w - 16, 16, h - 16, N)
        R.check_key_set("%s level %d distribute" % (name, l), sel, mine)
        total += len(cand)
    assert total > 0


@pytest.mark.parametrize("name", INPUTS)
def test_oracle_extract_same_bytes(name, oracle_mod):
    g, nf = _input(name)
    st = _stages(name)
    k, d = oracle_mod.orb_extract(g, nf)
    assert len(k) > 0
    R.check_records(name, k, d, st["kps"], st["desc"])
    assert k.tobytes() == st["kps"].tobytes() and d.tobytes() == st["desc"].tobytes()
    k2, d2 = R.orb_extract(g, nf)
    assert k2.tobytes() == st["kps"].tobytes() and d2.tobytes() == st["desc"].tobytes()


def test_inputs_take_the_paths_they_are_there_for():
    # low_contrast: contrast below iniTh everywhere, so every key comes from the minTh retry
    st = _stages("low_contrast")
    assert sum(len(c) for c in st["cands"]) > 0
    assert all(len(R.nms(R.fast_score_map(p, 20))) == 0 for p in st["pyramid"])
    # noise: far more candidates than the quota, so the sorted pass of the octree runs
    st = _stages("noise")
    assert len(st["cands"][0]) > 10 * st["cfg"]["n_per_level"][0]
    # kitti: the octree returns more than the quota on some level (the reference's behaviour)
    st = _stages("kitti0")
    assert len(st["kps"]) > 2000


def test_first_pass_overshoots_a_small_quota(oracle_mod):
    """DistributeOctTree keeps at most N + 2 keys once a pass starts below N, but the first pass
    makes up to 4 * nIni nodes whatever N is: a 1229 x 221 frame at 300 features (nIni 6-7, N 18
    on level 7) keeps more than N + 8 there, which the GPU's output slots must hold."""
    g = synthetic.gray_frame(221, 1229, 21)
    st = R.orb_stages(g, 300)
    over = []
    for l, (sel, N) in enumerate(zip(st["selected"], st["cfg"]["n_per_level"])):
        h, w = st["pyramid"][l].shape
        nini = R.n_ini(16, w - 16, 16, h - 16)
        assert len(sel) <= max(N + 2, 4 * nini)
        if len(sel) > N + 8:
            over.append(l)
    assert 7 in over
    k, d = oracle_mod.orb_extract(g, 300)
    R.check_records("1229x221", k, d, st["kps"], st["desc"])


def test_fast_atan2_bit_equal(oracle_mod):
    ys, xs = np.mgrid[-40:41, -40:41]
    pairs = list(zip(ys.ravel().tolist(), xs.ravel().tolist()))
    st = _stages("synth400x260")
    for l, sel in enumerate(st["selected"]):
        m01, m10 = R.ic_moments(st["pyramid"][l], sel[:, 0], sel[:, 1], st["cfg"]["umax"])
        pairs += list(zip(m01.tolist(), m10.tolist()))
    assert len(pairs) > 81 * 81 + 250
    y = np.array([p[0] for p in pairs], F)
    x = np.array([p[1] for p in pairs], F)
    mine = R.fast_atan2(y, x)
    theirs = np.array([oracle_mod.fast_atan2(float(a), float(b)) for a, b in zip(y, x)], F)
    bad = np.nonzero(mine.view(np.uint32) != theirs.view(np.uint32))[0]
    assert len(bad) == 0, "fastAtan2 differs at (y, x) = %s" % [(y[i], x[i]) for i in bad[:4]]


# ------------------------------------------------------------------ the comparisons can fail
def test_comparisons_catch_perturbed_inputs(oracle_mod):
    """Perturb what the restatement is given, or one value of what it returns, and every helper
    used above must report it (as test_map_invariants_catch_corruption does for the map)."""
    g, nf = _input("synth400x260")
    st = _stages("synth400x260")
    opyr = oracle_mod.pyramid(g)
    # one input pixel changed -> the restatement's pyramid differs from the oracle's of the original
    g2 = g.copy()
    g2[100, 200] ^= 0x40
    with pytest.raises(AssertionError, match="pyramid: level 0 differs in 1 px"):
        R.check_images("pyramid", R.pyramid(g2), opyr)
    with pytest.raises(AssertionError, match="from level 1: level 0 differs"):  # and it spreads down
        R.check_images("from level 1", R.pyramid(g2)[1:], opyr[1:])
    # one pixel of one pyramid level changed
    lv = [p.copy() for p in st["pyramid"]]
    lv[3][5, 7] += 1
    with pytest.raises(AssertionError, match=r"level 3 differs in 1 px, first \(y, x\) = \[5, 7\]"):
        R.check_images("pyramid", lv, opyr)
    with pytest.raises(AssertionError, match="blur: level 3 differs"):
        R.check_images("blur", [R.blur7(p) for p in lv], [oracle_mod.blur7(p) for p in opyr])
    # a candidate list with one response changed, two entries swapped, one entry dropped
    cand = oracle_mod.level_candidates(opyr[0])
    c2 = st["cands"][0].copy()
    c2[11, 2] += 1
    with pytest.raises(AssertionError, match="1 keys differ, first #11"):
        R.check_key_list("cands", cand, c2)
    with pytest.raises(AssertionError, match="only here"):
        R.check_key_set("cands", cand, c2)
    c2 = st["cands"][0].copy()
    c2[[4, 5]] = c2[[5, 4]]
    with pytest.raises(AssertionError, match="2 keys differ, first #4"):
        R.check_key_list("cands", cand, c2)
    R.check_key_set("cands", cand, c2)  # a set comparison does not see order
    with pytest.raises(AssertionError, match="against"):
        R.check_key_set("cands", cand, c2[1:])
    # the changed response reaches the octree's choice and the final records
    c2 = st["cands"][0].copy()
    sel = R.distribute(c2, 16, 400 - 16, 16, 260 - 16, 45)
    i = int(np.nonzero((c2 == sel[0]).all(1))[0][0])
    c2[i, 2] = 0  # the winner of its node loses (or, alone in its node, changes its response)
    with pytest.raises(AssertionError):
        R.check_key_set("distribute", sel, R.distribute(c2, 16, 400 - 16, 16, 260 - 16, 45))
    # final records: angle off by one ulp, one descriptor bit, one keypoint fewer
    k, d = oracle_mod.orb_extract(g, nf)
    k2 = st["kps"].copy()
    k2["angle"][17] = np.nextafter(k2["angle"][17], F(400))
    with pytest.raises(AssertionError, match="1 keypoint records differ, first #17"):
        R.check_records("extract", k, d, k2, st["desc"])
    d2 = st["desc"].copy()
    d2[3, 31] ^= 0x80
    with pytest.raises(AssertionError, match=r"1 descriptors differ \(first #3\)"):
        R.check_records("extract", k, d, st["kps"], d2)
    with pytest.raises(AssertionError, match="keypoints against"):
        R.check_records("extract", k, d, st["kps"][:-1], st["desc"][:-1])
    # and the perturbed image end to end
    k2, d2 = R.orb_extract(g2, nf)
    with pytest.raises(AssertionError):
        R.check_records("extract", k, d, k2, d2)
