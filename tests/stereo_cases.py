"""Image pairs shared by tests/test_stereo_ref_py.py and tests/test_gpu_stereo.py (and
tools/stereo_bench.py): a gray kitti_sample frame, its crop, and right images made from a left one
by a known disparity.  The restatement's result on a pair is computed once and shared."""
import functools
import os

import numpy as np

import orb_ref_py as R
import stereo_ref_py as S

KITTI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_sample")
BF = 387.5744  # Camera.bf of kitti03.yaml


@functools.lru_cache(maxsize=None)
def kitti_gray(i=0):
    """Frame i as 8-bit gray (integer BT.601 weights; any fixed gray image serves these tests)."""
    bgr = np.load(os.path.join(KITTI, "frame_%06d.npz" % i))["bgr"].astype(np.int64)
    g = (bgr[..., 0] * 1868 + bgr[..., 1] * 9617 + bgr[..., 2] * 4899 + 8192) >> 14
    g = np.ascontiguousarray(g.astype(np.uint8))
    g.setflags(write=False)
    return g


def crop():
    return np.ascontiguousarray(kitti_gray(0)[60:320, 400:800])


def add_noise(img, noise, seed):
    if not noise:
        return img
    rng = np.random.default_rng(seed)
    v = img.astype(np.int64) + rng.integers(-noise, noise + 1, img.shape)
    return np.clip(v, 0, 255).astype(np.uint8)


def shifted(left, d, noise=0, seed=7):
    """The right view of a fronto-parallel scene at disparity d: right[:, x] = left[:, x + d], the
    last column replicated, plus uniform +-noise grey levels."""
    h, w = left.shape
    cols = np.minimum(np.arange(w) + d, w - 1)
    return np.ascontiguousarray(add_noise(left[:, cols], noise, seed))


def banded(left, shifts=(3, 20, 60, 110)):
    """Four row bands of equal height, each at its own disparity."""
    h, w = left.shape
    out = np.empty_like(left)
    edges = np.linspace(0, h, len(shifts) + 1).astype(int)
    for d, a, b in zip(shifts, edges[:-1], edges[1:]):
        out[a:b] = shifted(left[a:b], d)
    return np.ascontiguousarray(out)


# name -> (left, right, nfeatures)
def pair(name):
    if name == "crop_s12_n3":
        return crop(), shifted(crop(), 12, 3), 500
    if name == "crop_s37_n0":
        return crop(), shifted(crop(), 37, 0), 500
    if name == "crop_s150_n3":
        return crop(), shifted(crop(), 150, 3), 500
    if name == "crop_identical":
        return crop(), crop(), 500
    if name == "kitti_banded":
        return kitti_gray(0), banded(kitti_gray(0)), 2000
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def stages(name, side):
    left, right, nf = pair(name)
    return R.orb_stages(left if side == 0 else right, nf)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement on a pair (shared: callers must not modify it)."""
    sl, sr = stages(name, 0), stages(name, 1)
    cfg = sl["cfg"]
    out = S.stereo_matches(sl["pyramid"], sr["pyramid"], sl["kps"], sl["desc"], sr["kps"],
                           sr["desc"], cfg["scale"], cfg["inv_scale"], BF)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ------------------------------------------------------------------ hand-placed keys
# A 320 x 240 pair, 8 levels.  The right image is the left one in four row bands, each at its own
# disparity and without noise, so that at level 0 the window search's answer is known exactly.
HAND_W, HAND_H = 320, 240
HAND_BANDS = ((0, 80, 20), (80, 120, 0), (120, 180, 197), (180, 240, 201))  # rows [a, b), shift


def texture(h, w, seed=5):
    """Seeded block noise at five scales: structure at every pyramid level."""
    rng = np.random.default_rng(seed)
    acc = np.zeros((h, w), np.int64)
    for k, amp in ((1, 40), (2, 40), (4, 50), (8, 60), (16, 60)):
        blk = rng.integers(0, amp, ((h + k - 1) // k, (w + k - 1) // k))
        acc += np.kron(blk, np.ones((k, k), np.int64))[:h, :w]
    return np.clip(acc, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def hand_pair():
    left = texture(HAND_H, HAND_W)
    rng = np.random.default_rng(11)
    # mirror-symmetric patch about column 160 (band 0-disparity): the SADs at shifts -1 and +1 are
    # equal, deltaR = 0, the disparity exactly 0
    for k in range(1, 13):
        left[92:109, 160 + k] = left[92:109, 160 - k]
    # ramp patch, rows 40..52, columns 95..106: every row is a_row + 7 * column, so the windows at
    # columns 100 and 101 are equal once their centre pixel is subtracted: two shifts tie at SAD 0
    a = rng.integers(20, 100, 13)
    left[40:53, 95:107] = (a[:, None] + 7 * np.arange(12)[None, :]).astype(np.uint8)
    # flat patch, rows 52..64, columns 44..76: every row constant, all eleven SADs are 0
    left[52:65, 44:77] = rng.integers(20, 200, 13).astype(np.uint8)[:, None]
    right = np.empty_like(left)
    for r0, r1, d in HAND_BANDS:
        right[r0:r1] = shifted(left[r0:r1], d)
    left.setflags(write=False)
    right.setflags(write=False)
    return left, right


def _flip(desc, k, rng):
    """desc with k distinct bits flipped: Hamming distance exactly k."""
    bits = np.unpackbits(desc)
    idx = rng.permutation(256)[:k]
    bits[idx] ^= 1
    return np.packbits(bits)


def _hand_spec():
    """[(tag, left (x, y, octave), [right (x, y, octave, flipped bits), ..])]; level-0 coordinates.
    The order fixes the key indices: the first right key is right key 0."""
    cfg = R.config(500)
    sc = cfg["scale"]
    F = np.float32
    up = lambda v: float(np.nextafter(F(v), F(np.inf)))    # noqa: E731
    dn = lambda v: float(np.nextafter(F(v), F(-np.inf)))   # noqa: E731
    spec = [
        ("key0", (150, 10, 0), [(130, 10, 0, 3)]),            # right key 0 wins: reported as -1
        ("tie", (150, 16, 0), [(130, 16, 0, 8), (100, 16, 0, 8)]),  # equal distances: lowest index
        ("no_cand", (150, 22, 0), []),                        # a row that lists no right key
        ("incl_hi", (250, 28, 0), [(250, 28, 0, 5)]),         # uR == uL
        ("incl_lo", (250, 34, 0), [(50, 34, 0, 6)]),          # uR == uL - 200
        ("excl_hi", (250, 46, 0), [(up(250), 46, 0, 5)]),     # one ulp right of uL
        ("excl_lo", (250, 52, 0), [(dn(50), 52, 0, 6)]),      # one ulp left of uL - 200
        ("d74", (150, 58, 0), [(130, 58, 0, 74)]),            # below thOrbDist: refined
        ("d75", (150, 64, 0), [(130, 64, 0, 75)]),            # at thOrbDist: not refined
        ("edge_eq", (312, 10, 0), [(309, 10, 0, 4)]),         # scaleduR0 + 11 == cols: skipped
        ("edge_in", (312, 16, 0), [(308, 16, 0, 4)]),         # scaleduR0 + 11 == cols - 1
        ("pinb", (100, 28, 0), [(9, 28, 0, 4)]),              # scaleduR0 - 10 < 0: pinned skip
        ("pinb_in", (100, 34, 0), [(10, 34, 0, 4)]),          # scaleduR0 - 10 == 0
        ("shift_m5", (200, 10, 0), [(185, 10, 0, 4)]),        # true match at incR = -5
        ("shift_p5", (200, 16, 0), [(175, 16, 0, 4)]),        # true match at incR = +5
        ("ramp", (100, 46, 0), [(80, 46, 0, 4)]),             # SADs tie at incR 0 and 1: delta 0.5
        ("flat", (60, 58, 0), [(40, 58, 0, 4)]),              # all eleven SADs equal: incR = -5
        ("clamp", (160, 100, 0), [(160, 100, 0, 2)]),         # disparity exactly 0
    ]
    # octave difference 2 (rejected) against 1 (accepted), left keys at level 2
    x2, y2 = float(F(60) * sc[2]), float(F(25) * sc[2])
    spec.append(("oct2", (x2, y2, 2), [(x2 - 20, y2, 0, 0), (x2 - 20, y2, 4, 0)]))
    # a matching key at every level, band of disparity 20, centred near (200, 40)
    for l in range(8):
        xl, yl = int(round(200 / float(sc[l]))), int(round(40 / float(sc[l])))
        x, y = float(F(xl) * sc[l]), float(F(yl) * sc[l])
        spec.append(("lvl%d" % l, (x, y, l), [(float(F(x) - F(20)), y, l, 2 + l)]))
    # level 7, key disparity 197.07: the band at 197 refines to just under 200, the band at 201 to
    # just over
    for tag, yl in (("under200", 42), ("over200", 59)):
        spec.append((tag, (float(F(75) * sc[7]), float(F(yl) * sc[7]), 7),
                     [(float(F(20) * sc[7]), float(F(yl) * sc[7]), 7, 3)]))
    return spec


HAND_SUBSETS = {
    "all": None,
    "accepted0": ("d75", "edge_eq", "shift_m5"),   # nothing accepted: pin (a)
    "accepted1": ("lvl3",),                         # median index 0
    "accepted2": ("lvl2", "lvl4"),                  # median index 1: the larger SAD
    "tied": ("key0", "lvl0", "d74", "lvl3"),       # SADs 0, 0, 0, s: median 0, all tied at thDist 0
}


@functools.lru_cache(maxsize=None)
def hand_case(subset="all"):
    """dict(left, right, kl, dl, kr, dr, tags (per left key), right_of (tag -> right indices))."""
    keep = HAND_SUBSETS[subset]
    rng = np.random.default_rng(23)
    kl, dl, kr, dr, tags, right_of = [], [], [], [], [], {}
    for tag, (x, y, o), rights in _hand_spec():
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        flipped = [_flip(d, nb, rng) for (_, _, _, nb) in rights]  # drawn whatever the subset
        if keep is not None and tag not in keep:
            continue
        tags.append(tag)
        kl.append((x, y, 31.0, 0.0, 1.0, o, -1))
        dl.append(d)
        right_of[tag] = list(range(len(kr), len(kr) + len(rights)))
        for (rx, ry, ro, _), fd in zip(rights, flipped):
            kr.append((rx, ry, 31.0, 0.0, 1.0, ro, -1))
            dr.append(fd)
    left, right = hand_pair()
    out = dict(left=left, right=right, kl=np.array(kl, R.KP_DTYPE),
               dl=np.array(dl, np.uint8).reshape(-1, 32), kr=np.array(kr, R.KP_DTYPE),
               dr=np.array(dr, np.uint8).reshape(-1, 32), tags=tags, right_of=right_of)
    return out


@functools.lru_cache(maxsize=None)
def hand_reference(subset="all"):
    c = hand_case(subset)
    cfg = R.config(500)
    out = S.stereo_matches(R.pyramid(c["left"], cfg), R.pyramid(c["right"], cfg), c["kl"], c["dl"],
                           c["kr"], c["dr"], cfg["scale"], cfg["inv_scale"], BF)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def hand_events(subset, out):
    """Assert that every event the hand-placed keys were chosen for shows in `out` (the
    restatement's result, or the library's)."""
    c = hand_case(subset)
    i = {t: k for k, t in enumerate(c["tags"])}
    r = c["right_of"]
    C = out["counters"]
    F = np.float32
    if subset == "accepted0":
        assert C["n_accepted"] == 0 and C["median"] == -1 and C["n_median_removed"] == 0
        assert C["n_window_edge"] == 1 and C["n_end_shift"] == 1 and C["n_coarse"] == 2
        return
    if subset == "accepted1":
        assert C["n_accepted"] == 1 and C["median"] == out["sad"][0] > 0
        assert C["n_median_removed"] == 0 and out["uR"][0] > 0
        return
    if subset == "accepted2":
        assert C["n_accepted"] == 2 and C["median"] == max(out["sad"]) and min(out["sad"]) > 0
        return
    if subset == "tied":
        assert C["n_accepted"] == 4 and sorted(out["sad"])[:3] == [0, 0, 0] and max(out["sad"]) > 0
        assert C["median"] == 0 and C["th_dist"] == 0 and C["n_median_removed"] == 4
        assert (out["uR"] == -1).all() and (out["right_idx"] == -1).all()
        return
    bd, sad, ridx, uR = out["best_dist"], out["sad"], out["right_idx"], out["uR"]
    # right key 0 wins and is refined, yet reported as -1
    assert r["key0"] == [0] and bd[i["key0"]] == 3 and sad[i["key0"]] == 0 and ridx[i["key0"]] == -1
    # equal Hamming distances: the lower index
    assert bd[i["tie"]] == 8 and ridx[i["tie"]] == r["tie"][0] and sad[i["tie"]] == 0
    assert bd[i["no_cand"]] == -1 and ridx[i["no_cand"]] == -1
    # octave difference 2 rejected, 1 accepted
    assert bd[i["oct2"]] == 100 and ridx[i["oct2"]] == -1
    assert bd[i["lvl3"]] == 5
    # the inclusive bounds of the search range, and one ulp outside
    assert bd[i["incl_hi"]] == 5 and bd[i["incl_lo"]] == 6
    assert bd[i["excl_hi"]] == 100 and bd[i["excl_lo"]] == 100
    # thOrbDist
    assert bd[i["d74"]] == 74 and sad[i["d74"]] == 0
    assert bd[i["d75"]] == 75 and sad[i["d75"]] == -1 and ridx[i["d75"]] == r["d75"][0]
    # the right border test, the pinned left one
    assert bd[i["edge_eq"]] == 4 and sad[i["edge_eq"]] == -1
    assert bd[i["edge_in"]] == 4 and sad[i["edge_in"]] >= 0
    assert bd[i["pinb"]] == 4 and sad[i["pinb"]] == -1
    assert bd[i["pinb_in"]] == 4 and sad[i["pinb_in"]] >= 0
    assert C["n_window_edge"] == 2
    # best shift at an end of the range; all SADs equal keeps the first shift
    for t in ("shift_m5", "shift_p5", "flat"):
        assert sad[i[t]] == 0 and out["depth"][i[t]] == -1, t
    assert C["n_end_shift"] >= 3
    # the parabola cannot leave [-0.5, 0.5] (the best SAD is below every earlier one and not above
    # any later one), so the delta test and a zero denominator are out of reach of the whole path
    assert C["n_delta"] == 0
    # disparity exactly 0
    assert C["n_clamped"] == 1 and sad[i["clamp"]] == 0
    assert uR[i["clamp"]] == F(160.0 - 0.01) and out["depth"][i["clamp"]] == F(BF) / F(0.01)
    # two shifts tie at the best SAD: the first wins, deltaR = 0.5
    assert sad[i["ramp"]] == 0 and uR[i["ramp"]] == F(80.5)
    # just under and just over 200 at level 7
    assert sad[i["under200"]] > 0 and sad[i["over200"]] > 0 and C["n_range"] >= 1
    xl7 = c["kl"]["x"][i["under200"]]
    assert 196 < xl7 - uR[i["under200"]] < 200 and out["depth"][i["over200"]] == -1
    assert C["n_accepted"] >= 10 and C["median"] >= 0
    assert sorted(set(c["kl"]["octave"].tolist())) == list(range(8))
