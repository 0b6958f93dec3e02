"""The NumPy restatement of the object front end (tests/objfront_ref_py.py) on cases worked out by
hand from the reference's lines, one or more per rule.  CPU only; the kernels, the host decisions
and the oracle are compared with the restatement elsewhere (test_gpu_objfront.py,
test_objdecide_host.py, test_oracle_objfront.py)."""
import numpy as np

import objfront_ref_py as R
import objfront_cases as C
from objfront_cases import decision_cases

F32 = np.float32


def test_a2_gray_and_depth():
    bgr = np.array([[[255, 255, 255], [255, 0, 0], [0, 0, 255], [0, 255, 0], [0, 0, 0]]], np.uint8)
    disp = np.array([[0, 1, 256, 65535, 128]], np.uint16)
    gray, depth = R.gray_depth(bgr, disp, 512.0)
    # (4899 c0 + 9617 c1 + 1868 c2 + 8192) >> 14: 255; 1257437 >> 14 = 76; 484532 >> 14 = 29;
    # 2460527 >> 14 = 150; 0
    assert gray.tolist() == [[255, 76, 29, 150, 0]]
    # 512 / (d / 256): d = 0 -> inf; 1 -> 131072; 256 -> 512; 128 -> 1024;
    # 65535 -> 512 / 255.99609375 = 2.00003051804..., the float next to it is 2 + 128 * 2^-22
    assert depth.dtype == np.float32
    assert depth.tolist() == [[np.inf, 131072.0, 512.0, float(F32(2.000030517578125)), 1024.0]]
    # dp is rounded to float before the division: d = 3, bf = 1: dp = 0.01171875 (exact),
    # 1 / 0.01171875 = 85.3333..., float 85.33333587646484
    assert R.gray_depth(bgr[:, :1], np.array([[3]], np.uint16), 1.0)[1][0, 0] == F32(256.0 / 3.0)


def _maps(W, H):
    return (np.full((H, W), 10, F32), np.full((H, W, 2), 1, F32), np.ones((H, W), np.int32))


def test_b1_comparisons_are_the_references():
    W, H = 12, 8
    depth, flow, mask = _maps(W, H)
    # grid positions (j, i): (0,0) (4,0) (8,0) (0,4) (4,4) (8,4)
    depth[0, 4] = 25.0                 # < 25 fails
    depth[0, 8] = 0.0                  # > 0 fails
    mask[4, 0] = 0                     # != 0 fails
    flow[4, 4] = (-4.0, 1.0)           # j + fx = 0: > 0 fails
    flow[4, 8] = (3.75, 3.5)           # 11.75 < 12, 7.5 < 8: kept
    mask[4, 8] = -5                    # != 0 holds for a negative label
    depth[1, 1] = 1.0                  # off the grid: never looked at
    o = R.object_samples(depth, flow, mask)
    assert o["count"] == 2
    assert o["keys"].tolist() == [[0, 0], [8, 4]]
    assert o["corres"].tolist() == [[1, 1], [11.75, 7.5]]
    assert o["flow"].tolist() == [[1, 1], [3.75, 3.5]]
    assert o["depth"].tolist() == [10, 10] and o["label"].tolist() == [1, -5]
    flow[4, 8] = (4.0, 3.5)            # j + fx = W: < cols fails
    assert R.object_samples(depth, flow, mask)["count"] == 1
    flow[4, 8] = (3.75, 4.0)           # i + fy = H
    assert R.object_samples(depth, flow, mask)["count"] == 1
    flow[0, 0] = (1.0, 0.0)            # i + fy = 0 at row 0
    assert R.object_samples(depth, flow, mask)["count"] == 0
    v = R.object_samples_vec(depth, flow, mask)
    assert v["count"] == 0 and v["keys"].shape == (0, 2)


def test_b2_comparisons_are_the_references():
    W, H = 12, 8
    depth, flow, mask = _maps(W, H)
    mask[:] = 0
    depth[2, 3], depth[3, 4] = 7.0, 0.0      # the truncated pixel and the rounded one of key 0
    mask[3, 4] = 2
    depth[1, 1] = 40.0                       # > 40 fails: kept
    depth[1, 2] = np.nextafter(F32(40), F32(50))
    depth[1, 3] = 0.0
    mask[1, 4] = 3                           # != 0: dropped
    flow[1, 5] = (0.0, 1.0)                  # one zero component: dropped
    flow[1, 6] = (1.0, 0.0)
    flow[1, 7] = (-20.0, -30.0)              # no lower bound: kept
    flow[1, 8] = (4.0, 1.0)                  # 8 + 4 = W: dropped
    flow[1, 9] = (1.0, 7.0)                  # 1 + 7 = H: dropped
    depth[1, 10] = np.inf                    # > 40: dropped
    keys = [(3.75, 2.75), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1), (9, 1),
            (10, 1), (11.5, 7.5),            # 11.5 + 1 = 12.5 is not < 12: dropped
            (10.5, 6.5)]
    o = R.static_samples(np.array(keys, F32), depth, flow, mask)
    assert o["count"] == 4
    assert o["keys"].tolist() == [[3.75, 2.75], [1, 1], [7, 1], [10.5, 6.5]]
    assert o["corres"].tolist() == [[4.75, 3.75], [2, 2], [-13, -29], [11.5, 7.5]]
    assert o["flow"].tolist() == [[1, 1], [1, 1], [-20, -30], [1, 1]]
    assert o["depth"].tolist() == [7, 40, 10, 10]   # mvSiftDepthTmp at the truncated key


def test_b4_round_is_half_away_from_zero_and_bounds_are_strict():
    assert R.c_round(np.array([0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997, 30.5, -0.4], F32)).tolist() == \
        [1, 2, 3, -1, -2, 0, 31, -0.0]
    assert np.isnan(R.c_round(F32(np.nan)))
    W, H = 8, 6
    depth = np.arange(W * H, dtype=F32).reshape(H, W) + 100
    mask = np.arange(W * H, dtype=np.int32).reshape(H, W) + 1
    depth[2, 3] = 0.0
    depth[2, 4] = -1.0
    keys = np.array([(0.5, 0.5),    # (1, 1): inside
                     (0.4, 3.0),    # column 0: outside
                     (3.0, 0.4),    # row 0: outside
                     (7.4, 5.4),    # (7, 5): the last pixel
                     (7.5, 3.0),    # column 8 = W: outside
                     (3.0, 5.5),    # row 6 = H: outside
                     (2.5, 1.5),    # (3, 2), not (2, 2): depth 0 there
                     (4.4, 2.4),    # (4, 2): depth -1
                     (np.nan, 2.0), (-0.5, 2.0)], F32)
    o = R.handoff(keys, keys, depth, mask)
    assert o["ns"] == o["no"] == 10
    assert np.array_equal(o["skeys"], keys, equal_nan=True) and np.array_equal(o["okeys"], keys, equal_nan=True)
    assert o["sdepth"].tolist() == [109, -1, -1, 147, -1, -1, -1, -1, -1, -1]
    assert o["odepth"].tolist() == [109, F32(0.1), F32(0.1), 147, F32(0.1), F32(0.1), 0, -1, F32(0.1), F32(0.1)]
    assert o["olabel"].tolist() == [10, 0, 0, 48, 0, 0, 20, 21, 0, 0]
    v = R.handoff_vec(keys, keys, depth, mask)
    for k in ("sdepth", "odepth", "olabel"):
        assert np.array_equal(o[k], v[k])


def test_b6_unprojection():
    K = (2.0, 4.0, 1.0, 1.0)  # invfx = 0.5, invfy = 0.25
    # Rlw: a quarter turn about y; tlw = (1, 2, 3).  key (3, 5), z = 2: x3Dc = (2, 2, 2);
    # Rwl = Rlw^T = [[0,0,-1],[0,1,0],[1,0,0]]; twl = -Rwl tlw = (3, -2, -1);
    # Rwl x3Dc = (-2, 2, 2); the world point is (1, 0, 1)
    T = np.array([[0, 0, 1, 1], [0, 1, 0, 2], [-1, 0, 0, 3], [0, 0, 0, 1]], F32)
    assert R.unproject_world(T, K, [(3, 5)], [2]).tolist() == [[1, 0, 1]]
    # x and y are float products: (u - cx) * z first, then * invfx.  u - cx = 1/3 (float),
    # z = 3: the float product is exactly 1 (0.3333333432674408 * 3 = 1.0000000298 -> 1.0)
    u = F32(1) + F32(1) / F32(3)
    assert R.unproject_world(np.eye(4), K, [(u, 1)], [3])[0].tolist() == \
        [float((u - F32(1)) * F32(3) * F32(0.5)), 0, 3]
    # cv::gemm accumulates in double: 2^24 + 1 - 2^24 = 1 (a float accumulator gives 0).
    # K = (1, 1, 0, 0): x3Dc = (u z, v z, z) = (2^24, 1, 2^24) for z = 2^24, u = 1, v = 2^-24
    T = np.eye(4, dtype=F32)
    T[:3, 0] = (1, 1, -1)  # Rwl's first row is Rlw's first column
    p = R.unproject_world(T, (1.0, 1.0, 0.0, 0.0), [(1.0, 2.0 ** -24)], [2.0 ** 24])
    assert p[0, 0] == 1.0
    # twl is a float matrix of its own, added in float: Rlw = I, tlw = (-2^24, 0, 0) gives
    # twl.x = 2^24; a point at x = 1 lands on float(1 + 2^24) = 2^24
    T = np.eye(4, dtype=F32)
    T[0, 3] = -2.0 ** 24
    assert R.unproject_world(T, (1.0, 1.0, 0.0, 0.0), [(1.0, 0.0)], [1.0])[0, 0] == 2.0 ** 24
    # a depth of inf (disparity 0) gives no finite point
    assert not np.isfinite(R.unproject_world(np.eye(4), K, [(3, 5)], [np.inf])).all()


def test_b6_scene_flow_norm_leaves_y_out():
    xc = np.array([[3, 100, 4], [0, 7, 0]], F32)
    xp = np.zeros((2, 3), F32)
    assert R.scene_flow_norm(xc, xp).tolist() == [5, 0]


def test_b7_statistics_in_posi_order():
    W, H, K, I = 200, 100, (100.0, 100.0, 100.0, 50.0), np.eye(4, dtype=F32)
    # nine samples of label 2, then the filtered ones
    ck = np.array([(100, 25), (100, 24.5), (100, 75), (100, 75.5), (50, 50), (49.5, 50), (150, 50),
                   (150.5, 50), (100, 50), (100, 50), (100, 50), (100, 50), (100, 50)], F32)
    cl = np.array([2, 2, 2, 2, 2, 2, 2, 2, 2, 0, -1, 2, 3], np.int32)
    ll = np.array([2, 2, 5, 5, 5, 2, 2, 2, 1, 2, 2, 0, -4], np.int32)
    cd = np.array([2.0 ** 24, 1, 1, 1, 1, 1, 1, 1, 1, 9, 9, 9, 9], F32)
    g = R.groups(ck, cd, cl, ck, cd, ll, I, I, K, W, H)
    assert g["obj_label"].tolist() == [-2] * 9 + [-1] * 4   # <= 0 on either side: -1
    assert g["members"][2].tolist() == list(range(9)) and len(g["members"][3]) == 0
    assert g["cnt"][2] == 9 and g["cnt"].sum() == 9
    assert g["bcnt"][2] == 4                                # the four keys past a line, none on one
    assert g["sfcnt"][2] == 9                               # nothing moved
    # sequential float sum: 2^24 + 1 stays 2^24, eight times over (any pairing of the ones first
    # would give more)
    assert g["depth_sum"][2] == 2.0 ** 24
    assert float(np.sum(cd[:9].astype(np.float64))) == 2.0 ** 24 + 8
    assert g["hist"][2].tolist() == [0, 1, 5, 0, 0, 3] + [0] * 10 and g["hist"].sum() == 9
    # the threshold is sf < 0.12f on sqrt(fx^2 + fz^2): move the last point by 0.5 in y only
    # (static) and by 0.5 in z only (moving)
    lk, ld = ck.copy(), cd[:].copy()
    ck2, cd2 = ck.copy(), np.full(13, 10, F32)
    ld[:] = 10
    ck2[8] = (100, 55)          # y = (55 - 50) * 10 / 100 = 0.5
    cd2[7] = 10.5               # z only: the key is the principal point, so x = y = 0
    ck2[7] = lk[7] = (100, 50)
    g = R.groups(ck2, cd2, cl, lk, ld, ll, I, I, K, W, H)
    assert g["sf"][8] == 0 and g["sf"][7] == 0.5
    assert g["sfcnt"][2] == 8


def test_b7_decisions_and_b8_on_the_hand_worked_cases():
    edges = [c for c in decision_cases() if c["expect"] is not None]
    assert len(edges) == 13
    for c in edges:
        got = R.decide(c["cnt"], c["bcnt"], c["sfcnt"], c["depth_sum"], c["hist"], c["bSecond"],
                       c["last_mod"], c["last_sem"])
        assert (list(got[0]), list(got[1])) == c["expect"], c["name"]


def test_vectorised_forms_equal_the_loops():
    """object_samples_vec and handoff_vec stand in for the loops on full-size inputs: on non-empty
    maps of the builder they give the loops' arrays bit for bit."""
    def same(a, b):
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for W, H, kind in ((37, 23, "random"), (37, 23, "edges"), (37, 23, "all"), (260, 200, "random")):
        c = C.object_case(W * 7 + H, W, H, kind)
        a = R.object_samples(c["depth"], c["flow"], c["mask"])
        b = R.object_samples_vec(c["depth"], c["flow"], c["mask"])
        assert a["count"] == b["count"] > 4, (W, H, kind)
        for k in ("keys", "corres", "flow", "depth", "label"):
            assert same(a[k], b[k]), (W, H, kind, k)
    for ns, no in ((22, 22), (700, 900)):
        c = C.handoff_case(5, ns, no)
        a = R.handoff(c["last_corres"], c["last_obj_corres"], c["depth"], c["mask"])
        b = R.handoff_vec(c["last_corres"], c["last_obj_corres"], c["depth"], c["mask"])
        assert (a["ns"], a["no"]) == (b["ns"], b["no"]) == (ns, no)
        assert (a["sdepth"] == -1).any() and (a["sdepth"] > 0).any() and (a["olabel"] == 0).any()
        for k in ("skeys", "sdepth", "okeys", "odepth", "olabel"):
            assert same(a[k], b[k]), (ns, no, k)


def test_b7_ratios_are_float32():
    # 30000002 / 100000000 = 0.30000002 > 0.3f = 0.3000000119... in double, but both counts are
    # floats and the float quotient rounds to 0.3f itself: not > 0.3f, the label is kept
    cnt, bcnt, sfcnt = (np.zeros(16, np.int32) for _ in range(3))
    cnt[1], sfcnt[1] = 100000000, 30000002
    assert 30000002 / 100000000 > float(F32(0.3))
    assert F32(30000002) / F32(100000000) == F32(0.3)
    hist = np.zeros((16, 16), np.int32)
    hist[1, 1] = 5
    kept, lab = R.decide(cnt, bcnt, sfcnt, np.zeros(16, F32), hist, False, [], [])
    assert kept == [1] and lab == [1]
