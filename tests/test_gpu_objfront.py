"""The object front end kernels (csrc/mmt_track.hip: k_gray_depth, k_static_samples, k_obj_count /
k_obj_write, k_handoff, k_obj_group), each run alone through its probe and compared EXACTLY --
every output array, bit for bit -- with the independent restatement tests/objfront_ref_py.py, at
the smallest shapes where each can still go wrong (tests/objfront_cases.py) and on the
kitti_sample frames.  Each case first asserts, on the restatement's output, the property it is
there for."""
import numpy as np
import pytest

import objfront_ref_py as R
import objfront_cases as C

pytestmark = pytest.mark.gpu

F32 = np.float32
BF = 387.5744


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(nfeatures=2000))
    yield c
    c.close()


def same(a, b):
    """Bit for bit: NaN equals the same NaN, -0.0 differs from 0.0."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xFF).all())


def check_samples(got, ref, cap, fields):
    """A sample set of capacity cap against the uncapped restatement: count = min(kept, cap), the
    first count entries are the restatement's first, the rest keeps the fill."""
    m = min(ref["count"], cap)
    assert got["count"] == m
    for k in fields:
        assert same(got[k][:m], ref[k][:m]), k
        assert untouched(got[k][m:]), k


# ------------------------------------------------------------------ A2
@pytest.mark.parametrize("W,H", [(8, 4), (7, 3), (5, 3), (40, 30), (37, 29), (45, 23)])
def test_gray_depth(ctx, W, H):
    assert (W * H) % 4 == {(8, 4): 0, (7, 3): 1, (5, 3): 3, (40, 30): 0, (37, 29): 1, (45, 23): 3}[(W, H)]
    bgr, disp = C.gray_depth_case(W * 100 + H, W, H, frames=2)
    rg, rz = R.gray_depth(bgr, disp, BF)
    # disparity 0 -> inf, 1 -> 256 bf, 65535 -> a little above bf / 256; also on the tail pixels
    assert np.isinf(rz[:, 0, 0]).all() and np.isinf(rz.reshape(2, -1)[:, -1]).all()
    assert (rz[:, 0, 1] == F32(BF) * 256).all() and (rz[:, 0, 2] > F32(BF) / 256).all()
    for pad in ((0, 0, 0, 0), (5, 3, 7, 1), (1, 1, 1, 1)):  # pitches 3WH and WH, then others
        g, z, gp, zp = ctx.gray_depth(bgr, disp, BF, pitch_pad=pad)
        assert same(g, rg) and same(z, rz), pad
        assert (gp == 0xA5).all() and (zp == 0xA5).all(), pad  # nothing written between frames


# ------------------------------------------------------------------ B2
STATIC_FIELDS = ("keys", "corres", "flow", "depth")


@pytest.fixture(scope="module")
def static_refs():
    out = {}
    for n in (0, 1, 4095, 4096, 4097, 9000):
        c = C.static_case(1000 + n, n)
        out[n] = (c, R.static_samples(np.stack([c["kps"]["x"], c["kps"]["y"]], 1), c["depth"],
                                      c["flow"], c["mask"]))
    return out


@pytest.mark.parametrize("n", [0, 1, 4095, 4096, 4097, 9000])  # one, two and three rounds
def test_static_samples(ctx, static_refs, n):
    c, ref = static_refs[n]
    kept = {(a, b) for a, b in ref["keys"].tolist()}
    for x, y, k in c["expect"]:  # depth 40 / just above / 0 / inf, labels, zero flow, x + fx = W...
        assert ((float(x), float(y)) in kept) == k, (x, y, k)
    if n >= 4095:
        assert ref["count"] > 1000 and len(c["expect"]) == 14
        assert (ref["corres"] < 0).any()
        assert (np.trunc(ref["keys"]) != np.round(ref["keys"])).any()
    got = ctx.static_samples(c["kps"], c["depth"], c["flow"], c["mask"], cap=n)
    check_samples(got, ref, n, STATIC_FIELDS)


@pytest.mark.parametrize("n,cap", [(4097, 100), (9000, 1024), (9000, -1), (4096, 0), (1, 0)])
def test_static_samples_truncated(ctx, static_refs, n, cap):
    c, ref = static_refs[n]
    cap = cap if cap >= 0 else ref["count"] - 1  # one short of everything
    assert cap < ref["count"]
    got = ctx.static_samples(c["kps"], c["depth"], c["flow"], c["mask"], cap=cap)
    assert got["count"] == cap
    check_samples(got, ref, cap, STATIC_FIELDS)


# ------------------------------------------------------------------ B1
OBJ_FIELDS = ("keys", "corres", "flow", "depth", "label")


@pytest.mark.parametrize("W,H,kind", [(20, 8, "random"), (20, 8, "all"), (20, 8, "none"),
                                      (37, 23, "random"), (37, 23, "all"), (37, 23, "none"),
                                      (37, 23, "edges"), (3, 2, "all"), (260, 200, "random")])
def test_object_samples(ctx, W, H, kind):
    c = C.object_case(W * 7 + H, W, H, kind)
    ref = R.object_samples(c["depth"], c["flow"], c["mask"])
    n = ((W + 3) // 4) * ((H + 3) // 4)  # 10 positions at 20 x 8: most of the 64 workgroups idle
    if kind == "all":
        assert ref["count"] == n
    elif kind == "none":
        assert ref["count"] == 0
    elif kind == "edges":
        kept = {(int(a), int(b)) for a, b in ref["keys"].tolist()}
        for (j, i), k in c["expect"].items():  # depth 25 / 0, j + fx = 0 / W, i + fy = 0 / H
            assert ((j, i) in kept) == k, (j, i, k)
    else:
        assert 0 < ref["count"] < n
    got = ctx.object_samples(c["depth"], c["flow"], c["mask"], cap=n)
    check_samples(got, ref, n, OBJ_FIELDS)
    if ref["count"] > 1:  # a truncated set
        cap = ref["count"] // 2
        got = ctx.object_samples(c["depth"], c["flow"], c["mask"], cap=cap)
        assert got["count"] == cap
        check_samples(got, ref, cap, OBJ_FIELDS)
    got = ctx.object_samples(c["depth"], c["flow"], c["mask"], cap=0)
    assert got["count"] == 0


def test_object_samples_full_size_order_across_workgroups(ctx):
    """1242 x 375: 457 grid positions per workgroup, two rounds of 256 each; kept runs laid over
    the first two workgroup boundaries come out in order and unbroken."""
    c = C.object_straddle_case(11)
    ref = R.object_samples_vec(c["depth"], c["flow"], c["mask"])
    assert c["per"] == 457
    keys = [tuple(int(v) for v in k) for k in ref["keys"].tolist()]
    a = keys.index(c["run"][0])
    assert keys[a:a + 12] == c["run"][:12]
    b = keys.index(c["run"][12])
    assert keys[b:b + 600] == c["run"][12:]
    n = 311 * 94
    got = ctx.object_samples(c["depth"], c["flow"], c["mask"], cap=n)
    check_samples(got, ref, n, OBJ_FIELDS)
    cap = b + 300  # the set ends inside the run, on the second workgroup boundary
    got = ctx.object_samples(c["depth"], c["flow"], c["mask"], cap=cap)
    assert got["count"] == cap
    check_samples(got, ref, cap, OBJ_FIELDS)


# ------------------------------------------------------------------ B4
@pytest.mark.parametrize("ns,no", [(0, 0), (1, 0), (0, 1), (1, 1), (8191, 8193), (8193, 8191),
                                   (22, 22)])
def test_sample_handoff(ctx, ns, no):
    c = C.handoff_case(ns * 3 + no, ns, no)
    ref = R.handoff(c["last_corres"], c["last_obj_corres"], c["depth"], c["mask"])
    for i, (u, v, inside) in enumerate(c["expect_o"]):  # x.5 either side of 0, round(u) in
        assert (ref["olabel"][i] != 0) == inside, (u, v)  # {0, 1, W-1, W}, NaN, ...
        assert (ref["odepth"][i] != F32(0.1)) == inside, (u, v)
    if ns >= 22:  # static keys over depth 0, depth < 0 and inf
        assert ref["sdepth"][19:22].tolist() == [-1, -1, np.inf]
        assert ref["sdepth"][0] > 0 and ref["sdepth"][1] == -1
    if no >= 22:
        assert ref["odepth"][19:22].tolist() == [0, -2, np.inf]
    got = ctx.sample_handoff(c["last_corres"], c["last_obj_corres"], c["depth"], c["mask"])
    assert got["ns"] == ns and got["no"] == no
    for k in ("skeys", "sdepth", "okeys", "odepth", "olabel"):
        assert same(got[k], ref[k]), k


# ------------------------------------------------------------------ B6 + B7 statistics
GROUP_ARGS = ("cur_keys", "cur_depth", "cur_label", "last_keys", "last_depth", "last_label", "Tcur",
              "Tlast", "K", "W", "H")
DEAD = [(0, 1), (-1, 2), (3, 0), (4, -3), (0, 0)]


def check_groups(ctx, c):
    ref = R.groups(*[c[k] for k in GROUP_ARGS])
    got = ctx.object_groups(*[c[k] for k in GROUP_ARGS])
    n = len(c["cur_depth"])
    assert got["err"] == 0
    assert same(got["obj_label"], ref["obj_label"])
    for k in ("cnt", "bcnt", "sfcnt", "hist"):
        assert same(got[k], ref[k]), k
    assert same(got["n_members"], ref["cnt"])
    for l in range(16):
        assert same(got["members"][l], ref["members"][l]), l
        assert untouched(got["members_raw"][l, len(ref["members"][l]):]), l
    assert same(got["depth_sum"], ref["depth_sum"]), (got["depth_sum"], ref["depth_sum"])
    assert n == 0 or got["obj_label"].shape == (n,)
    return ref


def check_kinds(c, ref):
    """The restatement on the case's deliberate samples: moves in y only are static, in z only are
    not; 0.119 is under the threshold and 0.121 over it; keys on a boundary line are inside."""
    live = ref["obj_label"] != -1
    sf, k = ref["sf"], c["kind"]
    assert (sf[live & (k == 2)] < F32(0.12)).all() and (sf[live & (k == 3)] > F32(0.12)).all()
    assert (sf[live & (k == 4)] < F32(0.12)).all() and (sf[live & (k == 5)] > F32(0.12)).all()
    assert (sf[live & (k == 1)] < F32(0.12)).all() and (sf[live & (k == 6)] > F32(0.12)).all()
    u, v = c["cur_keys"][:, 0], c["cur_keys"][:, 1]
    bnd = (v < 25) | (v > c["H"] - 25) | (u < 50) | (u > c["W"] - 50)
    for i, b in c["on_line"]:
        assert bool(bnd[i]) == b, i


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025])
def test_object_groups_sizes(ctx, n):
    sizes = {3: n - n // 3, 7: n // 3} if n > 1 else {3: n}
    c = C.group_case(300 + n, sizes, mixed_depth=n > 1)
    ref = check_groups(ctx, c)
    assert ref["cnt"].sum() == n
    if n > 1:
        check_kinds(c, ref)
        assert len(c["on_line"]) == 8 and c["orders_told_apart"] >= 1


def test_object_groups_member_counts_and_depth_chunks(ctx):
    """Labels of 0, 1, 511, 512, 513 and 1100 members (one to three chunks of the depth sum), dead
    samples (a label <= 0 on either side) in between, one current depth of inf."""
    c = C.group_case(41, {2: 1, 3: 511, 4: 512, 5: 513, 6: 1100}, extra=DEAD * 30, inf_label=3)
    ref = check_groups(ctx, c)
    assert ref["cnt"].tolist() == [0, 0, 1, 511, 512, 513, 1100] + [0] * 9
    assert (ref["obj_label"] == -1).sum() == 150
    assert np.isinf(ref["depth_sum"][3]) and np.isfinite(ref["depth_sum"][[4, 5, 6]]).all()
    # the sums tell summation orders apart: pairwise differs from sequential on these depths
    assert c["orders_told_apart"] >= 3
    check_kinds(c, ref)
    assert 0 < ref["sfcnt"][6] < 1100 and 0 < ref["bcnt"][6] < 1100
    assert (ref["hist"] != ref["hist"].T).any()


def test_object_groups_all_fifteen_labels(ctx):
    r = np.random.default_rng(5)
    sizes = {l: int(r.integers(5, 300)) for l in range(1, 16)}
    c = C.group_case(52, sizes, extra=DEAD * 5)
    ref = check_groups(ctx, c)
    assert (ref["cnt"][1:] == [sizes[l] for l in range(1, 16)]).all()
    check_kinds(c, ref)


def test_object_groups_image_smaller_than_the_boundary_band(ctx):
    """20 x 8: rows - 25 and cols - 50 are negative, every key is in the band."""
    c = C.group_case(70, {1: 200, 9: 130}, extra=DEAD * 4)
    c["W"], c["H"] = 20, 8
    ref = check_groups(ctx, c)
    assert ref["bcnt"].tolist() == ref["cnt"].tolist() and ref["cnt"][[1, 9]].tolist() == [200, 130]


@pytest.mark.parametrize("side", ["cur", "last"])
def test_object_groups_label_16_is_an_error_and_leaves_no_trace(ctx, side):
    import multimot_track_amd as M
    bad = C.group_case(60, {2: 40, 5: 40}, extra=[(16, 3) if side == "cur" else (3, 16)],
                       mixed_depth=False)
    with pytest.raises(ValueError):
        R.groups(*[bad[k] for k in GROUP_ARGS])
    with pytest.raises(M.MmtError, match=r"semantic label outside \[0, 15\]"):
        ctx.object_groups(*[bad[k] for k in GROUP_ARGS])
    good = C.group_case(61, {2: 40, 5: 40}, mixed_depth=False)  # the same context, clean again
    ref = check_groups(ctx, good)
    assert ref["cnt"][2] == ref["cnt"][5] == 40


# ------------------------------------------------------------------ real data
def test_front_end_probes_on_kitti_sample(ctx, kitti_frames):
    """The five probes over the fixture's frames, chained as the tracker chains them, with
    ctx.orb_extract keys: every output equals the restatement's."""
    from conftest import kitti_meta
    W, H = 1242, 375
    gt = [np.linalg.inv(np.asarray(p[1:], np.float64).reshape(4, 4)).astype(F32)
          for p in kitti_meta()["pose_gt"]]
    prev = None
    n_live = 0
    assert len(kitti_frames) == 5
    for t, f in enumerate(kitti_frames):
        rg, rz = R.gray_depth(f["bgr"], f["disp"], BF)
        g, z, _, _ = ctx.gray_depth(f["bgr"], f["disp"], BF)
        assert same(g[0], rg) and same(z[0], rz)
        kps = ctx.orb_extract(rg)[0]
        b2r = R.static_samples(np.stack([kps["x"], kps["y"]], 1), rz, f["flow"], f["sem"])
        check_samples(ctx.static_samples(kps, rz, f["flow"], f["sem"], cap=len(kps)), b2r,
                      len(kps), STATIC_FIELDS)
        b1r = R.object_samples_vec(rz, f["flow"], f["sem"])
        check_samples(ctx.object_samples(rz, f["flow"], f["sem"], cap=311 * 94), b1r, 311 * 94,
                      OBJ_FIELDS)
        assert b2r["count"] > 500 and b1r["count"] > 500
        if prev is not None:
            hr = R.handoff_vec(prev[0]["corres"], prev[1]["corres"], rz, f["sem"])
            hg = ctx.sample_handoff(prev[0]["corres"], prev[1]["corres"], rz, f["sem"])
            assert hg["ns"] == hr["ns"] and hg["no"] == hr["no"]
            for k in ("skeys", "sdepth", "okeys", "odepth", "olabel"):
                assert same(hg[k], hr[k]), k
            c = dict(cur_keys=hr["okeys"], cur_depth=hr["odepth"], cur_label=hr["olabel"],
                     last_keys=prev[1]["keys"], last_depth=prev[1]["depth"],
                     last_label=prev[1]["label"], Tcur=gt[t], Tlast=gt[t - 1], K=C.K_KITTI, W=W, H=H)
            ref = check_groups(ctx, c)
            n_live += int(ref["cnt"].sum())
        prev = (b2r, b1r)
    assert n_live > 2000  # four frame pairs
