"""mmt_stereo_matches / mmt_stereo_frame (csrc/mmt_stereo.hip) against the sequential restatement
tests/stereo_ref_py.py.  Every comparison is exact: uR and depth bit for bit, right_idx, best_dist,
sad and every counter equal.

1. Hand-placed keys (tests/stereo_cases.py, a 320 x 240 pair, 8 levels) through
   mmt_stereo_matches: tests/test_stereo_ref_py.py shows on the CPU that each event they were chosen
   for occurs in the restatement; here the same assertions run on the library's output.  Two events
   of the list cannot occur on the whole path and are covered at function level on the CPU only:
   the window search keeps the first smallest SAD, so d1 > d2 and d3 >= d2, the parabola's
   denominator is positive and deltaR lies in (-0.5, 0.5]: n_delta is 0, a zero denominator and a
   deltaR outside +-1 are unreachable.  The reachable end, deltaR = 0.5 from two tied SADs, is there.
2. Extracted keys through mmt_stereo_frame: the kitti_sample crop at 500 features (shift 12 and
   150 with noise, the identical pair) and frame 0 at full size, 2,000 features, four row bands.
3. Consistency of mmt_stereo_frame with mmt_orb_extract and mmt_stereo_matches, repeatability,
   sem_label.
4. Refusals.  A short capacity is refused with MMT_ENOSPC as by mmt_orb_extract: the counts are
   known only once the extraction has run, so that one follows the extraction (nothing is matched
   or copied); the others return before any launch.
"""
import numpy as np
import pytest

import multimot_track_amd as M
import orb_ref_py as R
import stereo_cases as C

pytestmark = pytest.mark.gpu

F = np.float32
MATCH_FIELDS = ("uR", "depth", "right_idx", "best_dist", "sad")


def _ctx(w, h, nf, max_batch=2):
    cfg = M.kitti03_config(w, h, nf, max_batch=max_batch)
    cfg.bf = C.BF
    return M.Context(cfg)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def check_matches(tag, got, ref, fields=MATCH_FIELDS):
    for f in fields:
        g, r = _bits(got[f]), _bits(ref[f])
        assert g.shape == r.shape, "%s: %s has %s entries against %s" % (tag, f, g.shape, r.shape)
        bad = np.nonzero(g != r)[0]
        assert len(bad) == 0, "%s: %s differs at %d keys, first #%d: %r against %r" % (
            tag, f, len(bad), bad[0], got[f][bad[0]], ref[f][bad[0]])
    gc, rc = got["counters"], ref["counters"]
    print(tag, gc)
    for k in rc:
        a, b = gc[k], rc[k]
        if k == "th_dist":
            a, b = F(a).view(np.uint32), F(b).view(np.uint32)
        assert a == b, "%s: counter %s is %r against %r (%s against %s)" % (tag, k, gc[k], rc[k],
                                                                           gc, rc)


# ------------------------------------------------------------------ 1. hand-placed keys
@pytest.fixture(scope="module")
def hand_ctx():
    ctx = _ctx(C.HAND_W, C.HAND_H, 500)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("subset", sorted(C.HAND_SUBSETS))
def test_hand_placed_keys(hand_ctx, subset):
    c = C.hand_case(subset)
    got = hand_ctx.stereo_matches(c["left"], c["right"], c["kl"], c["dl"], c["kr"], c["dr"])
    check_matches("hand " + subset, got, C.hand_reference(subset))
    C.hand_events(subset, got)


def test_no_keys(hand_ctx):
    """No left key, no right key, neither: empty outputs, zero counters, pin (a)."""
    c = C.hand_case("all")
    e_k, e_d = np.zeros(0, M.KP_DTYPE), np.zeros((0, 32), np.uint8)
    for kl, dl, kr, dr in ((e_k, e_d, c["kr"], c["dr"]), (c["kl"], c["dl"], e_k, e_d),
                           (e_k, e_d, e_k, e_d)):
        got = hand_ctx.stereo_matches(c["left"], c["right"], kl, dl, kr, dr)
        assert len(got["uR"]) == len(kl)
        assert (got["uR"] == -1).all() and (got["right_idx"] == -1).all()
        assert (got["best_dist"] == -1).all() and (got["sad"] == -1).all()
        cnt = got["counters"]
        assert cnt["median"] == -1 and cnt["th_dist"] == 0
        assert all(cnt[k] == 0 for k in M.STEREO_COUNTERS if k != "median")


# ------------------------------------------------------------------ 2. extracted keys
@pytest.fixture(scope="module")
def crop_ctx():
    ctx = _ctx(400, 260, 500)
    yield ctx
    ctx.close()


def _check_frame(tag, ctx, name):
    left, right, nf = C.pair(name)
    got = ctx.stereo_frame(left, right)
    sl, sr = C.stages(name, 0), C.stages(name, 1)
    R.check_records(tag + " left", got["kps"], got["desc"], sl["kps"], sl["desc"])
    R.check_records(tag + " right", got["kps_right"], got["desc_right"], sr["kps"], sr["desc"])
    check_matches(tag, got, C.reference(name), ("uR", "depth", "right_idx"))
    return got


@pytest.mark.parametrize("name", ["crop_s12_n3", "crop_s150_n3"])
def test_frame_shifted_crop(crop_ctx, name):
    got = _check_frame(name, crop_ctx, name)
    assert (got["uR"] >= 0).sum() >= 100


def test_frame_identical_crop(crop_ctx):
    got = _check_frame("identical", crop_ctx, "crop_identical")
    assert (got["uR"] == -1).all() and (got["depth"] == -1).all()
    assert got["counters"]["n_accepted"] == got["counters"]["n_median_removed"] == 254


@pytest.fixture(scope="module")
def kitti_ctx():
    ctx = _ctx(1242, 375, 2000)
    yield ctx
    ctx.close()


def test_frame_kitti_banded(kitti_ctx):
    got = _check_frame("kitti banded", kitti_ctx, "kitti_banded")
    assert (got["uR"] >= 0).sum() >= 450  # the restatement keeps 903


# ------------------------------------------------------------------ 3. consistency
def test_frame_consistency(crop_ctx):
    left, right, _ = C.pair("crop_s12_n3")
    mask = (np.arange(260)[:, None] * 1000 + np.arange(400)[None, :]).astype(np.int32)
    a = crop_ctx.stereo_frame(left, right, mask)
    kl, dl = crop_ctx.orb_extract(left)
    kr, dr = crop_ctx.orb_extract(right)
    assert a["kps"].tobytes() == kl.tobytes() and a["desc"].tobytes() == dl.tobytes()
    assert a["kps_right"].tobytes() == kr.tobytes() and a["desc_right"].tobytes() == dr.tobytes()
    m = crop_ctx.stereo_matches(left, right, kl, dl, kr, dr)
    check_matches("frame against matches", a, m, ("uR", "depth", "right_idx"))
    b = crop_ctx.stereo_frame(left, right, mask)
    for k in ("kps", "desc", "kps_right", "desc_right", "uR", "depth", "right_idx", "sem_label"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["counters"] == b["counters"]
    lab = kl["y"].astype(np.int64) * 1000 + kl["x"].astype(np.int64)
    assert (a["sem_label"] == lab).all()


def test_frame_without_left_keys(crop_ctx):
    """Frame.cc:103: no left key, the right count still reported."""
    flat = np.full((260, 400), 90, np.uint8)
    got = crop_ctx.stereo_frame(flat, C.crop())
    assert len(got["kps"]) == 0 and len(got["uR"]) == 0
    assert len(got["kps_right"]) == len(C.stages("crop_identical", 0)["kps"])
    assert got["counters"]["n_coarse"] == 0 and got["counters"]["median"] == -1


# ------------------------------------------------------------------ 4. refusals
def test_refusals(hand_ctx, crop_ctx):
    c = C.hand_case("accepted1")

    def matches(ctx, kl=c["kl"], kr=c["kr"]):
        return ctx.stereo_matches(c["left"], c["right"], kl, c["dl"], kr, c["dr"])
    one = _ctx(C.HAND_W, C.HAND_H, 500, max_batch=1)
    for call in (lambda: matches(one), lambda: one.stereo_frame(c["left"], c["right"])):
        with pytest.raises(M.MmtError, match="-22.*max_batch >= 2"):
            call()
    one.close()
    for side, field, value in (("l", "x", 3.0), ("l", "octave", 8), ("r", "octave", 8),
                               ("r", "y", 1.0), ("l", "octave", -1)):
        k = (c["kl"] if side == "l" else c["kr"]).copy()
        k[field][0] = value
        with pytest.raises(M.MmtError, match="-22"):
            matches(hand_ctx, **({"kl": k} if side == "l" else {"kr": k}))
    left, right, _ = C.pair("crop_s12_n3")
    with pytest.raises(M.MmtError, match="-28"):
        crop_ctx.stereo_frame(left, right, cap=100)
    # the context still works
    check_matches("after refusals", matches(hand_ctx), C.hand_reference("accepted1"))
