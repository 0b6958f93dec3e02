"""Seeded inputs for the object front end tests (test_gpu_objfront.py, test_objdecide_host.py):
the smallest shapes at which each kernel of csrc/mmt_track.hip's front end can still go wrong, and
the decision cases of csrc/mmt_objdecide.cpp.  Each builder returns plain arrays plus the facts the
case is there for (`expect`), which the tests assert on the restatement's output before they
compare the kernel with it."""
import numpy as np

F32 = np.float32
K_KITTI = (721.5377, 721.5377, 609.5593, 172.8540)
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])  # mmt_kp
UP40 = np.nextafter(F32(40), F32(100))
UP25 = np.nextafter(F32(25), F32(100))


# ------------------------------------------------------------------ A2
def gray_depth_case(seed, W, H, frames=2):
    r = np.random.default_rng(seed)
    bgr = r.integers(0, 256, (frames, H, W, 3), dtype=np.uint8)
    disp = r.integers(1, 65536, (frames, H, W)).astype(np.uint16)
    flat = disp.reshape(frames, -1)
    flat[:, 0], flat[:, 1], flat[:, 2] = 0, 1, 65535
    flat[:, -1] = 0  # the tail pixel of an odd-sized frame
    flat[:, -2] = 65535
    return bgr, disp


# ------------------------------------------------------------------ maps shared by B1 / B2 / B4
def random_maps(r, W, H, flow_span, depth_hi=60):
    depth = r.uniform(0.5, depth_hi, (H, W)).astype(F32)
    depth[r.random((H, W)) < 0.05] = 0
    depth[r.random((H, W)) < 0.02] = -1
    flow = r.uniform(-flow_span, flow_span, (H, W, 2)).astype(F32)
    flow[r.random((H, W)) < 0.05, 0] = 0
    flow[r.random((H, W)) < 0.05, 1] = 0
    mask = r.integers(0, 4, (H, W)).astype(np.int32)
    mask[r.random((H, W)) < 0.5] = 0
    return depth, flow, mask


# ------------------------------------------------------------------ B2
STATIC_W, STATIC_H = 64, 48


def static_case(seed, n):
    """n keys on a 64 x 48 image; the first keys are the special ones (as many as fit in n), each
    on a pixel of its own in row 2 * k + 1, with `expect[k]` = kept or not."""
    r = np.random.default_rng(seed)
    W, H = STATIC_W, STATIC_H
    depth, flow, mask = random_maps(r, W, H, 20)
    sp = []  # (x, y, depth, label, flow, kept)

    def special(x, d, lab, fl, kept):
        y = 2 * len(sp) + 1.0
        sp.append((x, y, kept))
        depth[int(y), int(x)], mask[int(y), int(x)], flow[int(y), int(x)] = d, lab, fl

    special(5.0, 40.0, 0, (1.5, 1.5), True)       # depth exactly 40: > 40 is false
    special(5.0, UP40, 0, (1.5, 1.5), False)      # just above 40
    special(5.0, 0.0, 0, (1.5, 1.5), False)       # depth 0
    special(5.0, np.inf, 0, (1.5, 1.5), False)    # depth inf (disparity 0)
    special(5.0, 10.0, 2, (1.5, 1.5), False)      # labelled pixel
    special(5.0, 10.0, -1, (1.5, 1.5), False)     # a negative label is != 0 too
    special(5.0, 10.0, 0, (0.0, 1.5), False)      # exactly one zero flow component
    special(5.0, 10.0, 0, (1.5, 0.0), False)
    special(10.0, 10.0, 0, (W - 10.0, 1.5), False)   # x + fx exactly W
    special(10.0, 10.0, 0, (W - 10.5, 1.5), True)    # x + fx just inside
    special(10.0, 10.0, 0, (-30.0, -40.0), True)     # negative correspondence: no lower bound
    special(10.0, 10.0, 0, (1.5, H - (2 * len(sp) + 1.0)), False)   # y + fy exactly H
    special(10.0, 10.0, 0, (1.5, H - (2 * len(sp) + 1.5)), True)    # y + fy just inside
    # fractional key: truncation reads pixel (12, y), rounding would read (13, y + 1)
    x, y = 12.75, 2 * len(sp) + 1.75
    sp.append((x, y, True))
    depth[int(y), 12], mask[int(y), 12], flow[int(y), 12] = 7.0, 0, (2.25, -0.5)
    depth[int(y) + 1, 13], mask[int(y) + 1, 13] = 0.0, 3
    depth[int(y), 13], mask[int(y), 13] = 0.0, 3
    kps = np.zeros(n, KP_DTYPE)
    kps["x"] = r.uniform(0, W, n).astype(F32).clip(0, np.nextafter(F32(W), F32(0)))
    kps["y"] = r.uniform(0, H, n).astype(F32).clip(0, np.nextafter(F32(H), F32(0)))
    taken = {(int(a), int(b)) for a, b, _ in sp}
    for i in range(n):  # random keys stay off the specials' pixels
        while (int(kps["x"][i]), int(kps["y"][i])) in taken:
            kps["x"][i] = F32(r.uniform(0, W - 1))
            kps["y"][i] = F32(r.uniform(0, H - 1))
    m = min(n, len(sp))
    for k in range(m):
        kps["x"][k], kps["y"][k] = sp[k][0], sp[k][1]
    return dict(kps=kps, depth=depth, flow=flow, mask=mask,
                expect=[(F32(sp[k][0]), F32(sp[k][1]), sp[k][2]) for k in range(m)])


# ------------------------------------------------------------------ B1
def object_case(seed, W, H, kind="random"):
    """kind: random | all (every grid position kept) | none (every one rejected, each for a
    different reason) | edges (hand-placed grid positions, `expect` = {(j, i): kept})."""
    r = np.random.default_rng(seed)
    depth, flow, mask = random_maps(r, W, H, 3, depth_hi=35)
    expect = {}
    if kind == "all":
        depth[:] = r.uniform(1, 24, (H, W))
        mask[:] = r.integers(1, 4, (H, W))
        flow[:] = r.uniform(0.25, 0.75, (H, W, 2))  # i + 0.25 > 0 even at i = 0; < H for H % 4 != 1
    elif kind == "none":
        q = np.arange(W * H).reshape(H, W) % 4
        depth[:] = r.uniform(1, 24, (H, W))
        mask[:] = 1
        flow[:] = 0.5
        mask[q == 0] = 0
        depth[q == 1] = 25
        depth[q == 2] = 0
        flow[q == 3, 0] = -W
    elif kind == "edges":
        def put(j, i, d, lab, fl, kept):
            depth[i, j], mask[i, j], flow[i, j] = d, lab, fl
            expect[(j, i)] = kept
        put(4, 4, 25.0, 1, (1, 1), False)        # depth exactly 25: < 25 is false
        put(8, 4, np.nextafter(F32(25), F32(0)), 1, (1, 1), True)
        put(12, 4, 0.0, 1, (1, 1), False)        # depth 0: > 0 is false
        put(16, 4, 1e-30, 2, (1, 1), True)
        put(4, 8, 10.0, 1, (-4.0, 1), False)     # j + fx exactly 0
        put(8, 8, 10.0, 1, (-7.75, 1), True)     # 0.25
        put(12, 8, 10.0, 1, (W - 12.0, 1), False)   # j + fx exactly W
        put(16, 8, 10.0, 3, (W - 16.5, 1), True)
        put(4, 12, 10.0, 1, (1, -12.0), False)   # i + fy exactly 0
        put(8, 12, 10.0, 1, (1, H - 12.0), False)   # i + fy exactly H
        put(12, 12, 10.0, -2, (1, 1), True)      # a negative label is != 0
        put(16, 12, 10.0, 0, (1, 1), False)
        put(0, 0, 10.0, 1, (0.5, 0.5), True)     # the corner position
        put(0, 4, 10.0, 1, (0.0, 0.5), False)    # column 0 with no x flow: 0 > 0 is false
    return dict(depth=depth, flow=flow, mask=mask, expect=expect)


def object_straddle_case(seed, W=1242, H=375):
    """Full-size image; grid positions [per - 6, per + 6) and [2 per - 300, 2 per + 300) are all
    kept, so kept runs cross the first two workgroup boundaries and a 256-position round."""
    c = object_case(seed, W, H)
    gw, gh = (W + 3) // 4, (H + 3) // 4
    per = (gw * gh + 63) // 64
    run = list(range(per - 6, per + 6)) + list(range(2 * per - 300, 2 * per + 300))
    for g in run:
        i, j = (g // gw) * 4, (g % gw) * 4
        c["depth"][i, j], c["mask"][i, j], c["flow"][i, j] = 5.0 + (g % 7), 1 + g % 3, (0.5, 0.5)
    c["run"] = [((g % gw) * 4, (g // gw) * 4) for g in run]
    c["per"] = per
    return c


# ------------------------------------------------------------------ B4
HANDOFF_W, HANDOFF_H = 32, 24


def handoff_case(seed, ns, no):
    """Keys around a 32 x 24 image.  The first keys of both lists are the special ones; `expect`
    lists (u, v, inside) for them."""
    r = np.random.default_rng(seed)
    W, H = HANDOFF_W, HANDOFF_H
    depth, _, mask = random_maps(r, W, H, 1)
    mask[mask == 0] = 7  # every pixel labelled, so the outside value 0 is told apart
    nan = np.nan
    sp = [(0.5, 5.0, True),          # round(0.5) = 1: half away from zero (half-to-even gives 0)
          (-0.5, 5.0, False),        # -1
          (0.49999997, 5.0, False),  # 0: column 0 is outside
          (1.5, 2.5, True),          # (2, 3)
          (2.5, 4.5, True),          # (3, 5), not (2, 4)
          (-1.5, 5.0, False),
          (W - 1.5, 5.0, True),      # W - 1 (30.5 rounds up to 31)
          (W - 0.5, 5.0, False),     # W
          (W - 0.50001, 5.0, True),  # W - 1
          (5.0, 0.4, False),         # row 0 is outside
          (5.0, 0.5, True),          # row 1
          (5.0, H - 0.5, False),     # row H
          (5.0, H - 1.4, True),      # row H - 1
          (nan, 5.0, False), (5.0, nan, False), (nan, nan, False),
          (1e30, 5.0, False), (5.0, -1e30, False), (np.inf, 5.0, False),
          (7.3, 9.6, True), (8.3, 9.6, True), (9.3, 9.6, True)]
    depth[10, 7], depth[10, 8], depth[10, 9] = 0.0, -2.0, np.inf  # under the last three keys
    depth[5, 1] = 12.5  # under the first one

    def keys(n):
        k = np.stack([r.uniform(-3, W + 3, n), r.uniform(-3, H + 3, n)], 1).astype(F32)
        half = r.random(n) < 0.25  # many keys at x.5
        k[half] = np.floor(k[half]) + F32(0.5)
        m = min(n, len(sp))
        k[:m] = np.array([(a, b) for a, b, _ in sp[:m]], F32).reshape(-1, 2)
        return k, [(F32(a), F32(b), c) for a, b, c in sp[:m]]

    sk, es = keys(ns)
    ok, eo = keys(no)
    return dict(last_corres=sk, last_obj_corres=ok, depth=depth, mask=mask, expect_s=es, expect_o=eo)


# ------------------------------------------------------------------ B6 + B7 statistics
GROUP_W, GROUP_H = 1242, 375


def _pose(r, scale):
    w = r.normal(0, 0.03 * scale, 3)
    th = np.linalg.norm(w)
    k = w / max(th, 1e-12)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = r.normal(0, 0.5 * scale, 3)
    return T.astype(F32)


def sf64(c, idx=None):
    """Scene flow norm of the case's samples in float64 from the float32 inputs (the builder's own
    arithmetic, for the distance-from-threshold condition)."""
    fx, fy, cx, cy = K_KITTI

    def world(T, k, z):
        T = T.astype(np.float64)
        z = z.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            X = np.stack([(k[:, 0] - F32(cx)).astype(np.float64) * z / fx,
                          (k[:, 1] - F32(cy)).astype(np.float64) * z / fy, z], 1)
            return (X - T[:3, 3]) @ T[:3, :3]
    with np.errstate(invalid="ignore", over="ignore"):
        d = world(c["Tcur"], c["cur_keys"], c["cur_depth"]) - world(c["Tlast"], c["last_keys"], c["last_depth"])
        return np.sqrt(d[:, 0] ** 2 + d[:, 2] ** 2)


def group_case(seed, sizes, extra=(), mixed_depth=True, inf_label=None):
    """sizes: {label: members}.  extra: (cur_label, last_label) pairs of further samples (the <= 0
    and the out-of-range ones).  Every live sample is one of the kinds of `kind` below; the
    positions are a seeded shuffle.  Returns the arrays, `kind` per sample, and asserts the two
    builder conditions (distance from the sf threshold; depth sums that tell orders apart)."""
    r = np.random.default_rng(seed)
    W, H = GROUP_W, GROUP_H
    fx, fy, cx, cy = K_KITTI
    Tlast, Tcur = _pose(r, 1.0), _pose(r, 1.0)
    cl = np.array([l for l, m in sizes.items() for _ in range(m)] + [e[0] for e in extra], np.int32)
    n = len(cl)
    ll = cl.copy()
    swap = r.random(n) < 0.3
    ll[swap] = r.integers(1, 16, int(swap.sum()))
    for k, e in enumerate(extra):
        ll[n - len(extra) + k] = e[1]
    perm = r.permutation(n)
    cl, ll = cl[perm], ll[perm]
    # kinds: 0 unrelated (large flow), 1 rigid static (|dX| <= 0.05), 2 moves in y only,
    # 3 moves in z only, 4 sf = 0.119, 5 sf = 0.121, 6 moves 0.3..2 in x and z
    kind = r.choice(7, n, p=[0.3, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1])
    lk = np.stack([r.uniform(0, W, n), r.uniform(0, H, n)], 1).astype(F32)
    ld = r.uniform(3, 60, n).astype(F32)
    Tl, Tc = Tlast.astype(np.float64), Tcur.astype(np.float64)
    Xl = np.stack([(lk[:, 0] - cx) * ld / fx, (lk[:, 1] - cy) * ld / fy, ld], 1).astype(np.float64)
    Xw = (Xl - Tl[:3, 3]) @ Tl[:3, :3]
    ang = r.uniform(0, 2 * np.pi, n)
    mag = np.select([kind == 1, kind == 4, kind == 5, kind == 6],
                    [r.uniform(0, 0.05, n), 0.119, 0.121, r.uniform(0.3, 2, n)], 0.0)
    dX = np.stack([mag * np.cos(ang), r.uniform(-0.3, 0.3, n), mag * np.sin(ang)], 1)
    dX[kind == 2] = np.stack([np.zeros(n), r.uniform(0.3, 1, n), np.zeros(n)], 1)[kind == 2]
    dX[kind == 3] = np.stack([np.zeros(n), np.zeros(n), r.uniform(0.3, 1, n)], 1)[kind == 3]
    Xc = (Xw + dX) @ Tc[:3, :3].T + Tc[:3, 3]
    Xc[:, 2] = np.maximum(Xc[:, 2], 0.5)
    ck = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1).astype(F32)
    cd = Xc[:, 2].astype(F32)
    un = kind == 0
    ck[un] = np.stack([r.uniform(0, W, n), r.uniform(0, H, n)], 1).astype(F32)[un]
    cd[un] = (10.0 ** r.uniform(-2, 4, n)).astype(F32)[un] if mixed_depth else r.uniform(1, 50, n).astype(F32)[un]
    # keys exactly on, and one float past, the four boundary lines (unrelated samples only)
    lines = [(50.0, 100.0, False), (np.nextafter(F32(50), F32(0)), 100.0, True),
             (W - 50.0, 100.0, False), (np.nextafter(F32(W - 50), F32(1e9)), 100.0, True),
             (600.0, 25.0, False), (600.0, np.nextafter(F32(25), F32(0)), True),
             (600.0, H - 25.0, False), (600.0, np.nextafter(F32(H - 25), F32(1e9)), True)]
    live = np.nonzero(un & (cl > 0) & (cl < 16) & (ll > 0) & (ll < 16))[0]
    on_line = []
    for (u, v, b), i in zip(lines, live):
        ck[i] = (u, v)
        on_line.append((int(i), b))
    c = dict(cur_keys=ck, cur_depth=cd, cur_label=cl, last_keys=lk, last_depth=ld, last_label=ll,
             Tcur=Tcur, Tlast=Tlast, K=K_KITTI, W=W, H=H, kind=kind, on_line=on_line)
    if inf_label is not None:
        i = np.nonzero(un & (cl == inf_label) & (ll > 0))[0][0]
        cd[i] = np.inf
        c["inf_at"] = int(i)
    # ---- builder condition 1: distance from the sf threshold
    s = sf64(c)
    livem = (cl > 0) & (ll > 0)
    near = livem & (np.abs(s - 0.12) < 1e-3)
    assert not (near & (kind != 4) & (kind != 5)).any(), "seed puts a sample at the sf threshold"
    assert (np.abs(s[livem & (kind == 4)] - 0.119) < 2e-4).all()
    assert (np.abs(s[livem & (kind == 5)] - 0.121) < 2e-4).all()
    # ---- builder condition 2: depth sums that tell summation orders apart
    if mixed_depth:
        told = 0
        for l in range(1, 16):
            d = cd[livem & (cl == l)]
            if len(d) > 8 and np.isfinite(d).all():
                told += int(np.sum(d, dtype=F32) != np.add.accumulate(d, dtype=F32)[-1])
        c["orders_told_apart"] = told
    return c


# ------------------------------------------------------------------ B7 decisions + B8
def _dec(name, labels, bSecond=False, last_mod=(), last_sem=(), expect=None):
    """labels: {l: dict(cnt, bcnt, sfcnt, depth_sum, hist={last label: count})}."""
    cnt, bcnt, sfcnt = (np.zeros(16, np.int32) for _ in range(3))
    ds = np.zeros(16, F32)
    hist = np.zeros((16, 16), np.int32)
    for l, s in labels.items():
        cnt[l], bcnt[l], sfcnt[l] = s["cnt"], s.get("bcnt", 0), s.get("sfcnt", 0)
        ds[l] = F32(s.get("depth_sum", 10.0 * s["cnt"]))
        for k, v in s.get("hist", {l: s["cnt"]}).items():
            hist[l, k] = v
    return dict(name=name, cnt=cnt, bcnt=bcnt, sfcnt=sfcnt, depth_sum=ds, hist=hist,
                bSecond=bSecond, last_mod=list(last_mod), last_sem=list(last_sem), expect=expect)


def decision_cases():
    """The edge cases, each with the decision worked out by hand (`expect` = (kept labels,
    LabId)), then 200 seeded random ones (expect None)."""
    ok = dict(cnt=200)
    assert F32(300) / F32(1000) == F32(0.3) and F32(301) / F32(1000) > F32(0.3)
    up3200 = np.nextafter(F32(3200), F32(1e9))
    C = [
        _dec("boundary share 0.5 kept, above dropped",
             {1: dict(cnt=200, bcnt=100), 2: dict(cnt=200, bcnt=101), 3: dict(cnt=201, bcnt=101)},
             expect=([1], [1])),
        _dec("cnt 100 dropped, 101 kept", {1: dict(cnt=100), 2: dict(cnt=101)}, expect=([2], [1])),
        _dec("sfcnt/cnt == 0.3f kept, one more dropped",
             {4: dict(cnt=1000, sfcnt=300), 5: dict(cnt=1000, sfcnt=301)}, expect=([4], [1])),
        _dec("mean depth exactly 25 kept, one float above dropped",
             {1: dict(cnt=128, depth_sum=3200.0), 2: dict(cnt=128, depth_sum=up3200)},
             expect=([1], [1])),
        _dec("empty label between kept ones", {1: ok, 2: dict(cnt=0), 3: ok},
             last_mod=[5, 6], last_sem=[1, 3], expect=([1, 3], [5, 6])),
        _dec("all 15 labels kept", {l: ok for l in range(1, 16)}, last_mod=[3], last_sem=[9],
             expect=(list(range(1, 16)), [4, 5, 6, 7, 8, 9, 10, 11, 3, 12, 13, 14, 15, 16, 17])),
        _dec("bSecond numbers from 1 whatever the last frame had", {2: ok, 7: ok, 9: ok},
             bSecond=True, last_mod=[40, 41], last_sem=[2, 7], expect=([2, 7, 9], [1, 2, 3])),
        _dec("max + 1 numbering; New_lab absent from the last nSemPosition",
             {3: ok, 5: ok}, last_mod=[4, 7], last_sem=[1, 2], expect=([3, 5], [8, 9])),
        _dec("two objects choose the same last label",
             {1: dict(cnt=200, hist={2: 150, 1: 50}), 2: dict(cnt=300, hist={2: 300})},
             last_mod=[6, 9], last_sem=[1, 2], expect=([1, 2], [9, 9])),
        _dec("histogram tie: the smaller last label wins",
             {4: dict(cnt=200, hist={5: 80, 2: 80, 9: 40})}, last_mod=[11, 12, 13],
             last_sem=[5, 2, 9], expect=([4], [12])),
        _dec("histogram tie the other way round is not a tie",
             {4: dict(cnt=200, hist={5: 81, 2: 80, 9: 39})}, last_mod=[11, 12, 13],
             last_sem=[5, 2, 9], expect=([4], [11])),
        _dec("empty last nModLabel: new labels from 1 (the project's pin)", {1: ok, 2: ok},
             expect=([1, 2], [1, 2])),
        _dec("nothing kept", {1: dict(cnt=50), 2: dict(cnt=300, sfcnt=200)}, last_mod=[2],
             last_sem=[1], expect=([], [])),
    ]
    r = np.random.default_rng(20240607)
    for k in range(200):
        labels = {}
        for l in range(1, 16):
            if r.random() < 0.4:
                continue
            cnt = int(r.choice([0, 1, 99, 100, 101, 102, 128, 200, 1000, int(r.integers(1, 3000))]))
            if cnt == 0:
                labels[l] = dict(cnt=0, hist={})
                continue
            bcnt = int(r.choice([0, cnt // 2, cnt // 2 + 1, int(r.integers(0, cnt + 1))]))
            sfcnt = int(r.choice([0, (3 * cnt) // 10, (3 * cnt) // 10 + 1, int(r.integers(0, cnt + 1))]))
            mean = float(r.choice([5.0, 25.0, 25.000002, 24.999998, r.uniform(1, 40)]))
            parts = r.multinomial(cnt, r.dirichlet(np.ones(4)))
            lls = r.choice(np.arange(1, 16), 4, replace=False)
            if r.random() < 0.3:
                parts[1] = parts[0]  # a tie (the counts need not add up to cnt for the decision)
            labels[l] = dict(cnt=cnt, bcnt=bcnt, sfcnt=sfcnt, depth_sum=F32(mean) * F32(cnt),
                             hist={int(a): int(b) for a, b in zip(lls, parts) if b > 0} or {1: cnt})
        m = int(r.integers(0, 6))
        sem = r.choice(np.arange(1, 16), m, replace=False).tolist()
        mod = r.integers(1, 30, m).tolist()
        C.append(_dec("random %d" % k, labels, bSecond=bool(r.random() < 0.15), last_mod=mod,
                      last_sem=sem))
    return C


def write_decision_cases(path, cases):
    """The input file of tests/objdecide_host_check.cpp."""
    with open(path, "w") as f:
        f.write("%d\n" % len(cases))
        for c in cases:
            f.write("%d %d\n" % (int(c["bSecond"]), len(c["last_mod"])))
            f.write(" ".join(str(v) for v in c["last_mod"]) + "\n")
            f.write(" ".join(str(v) for v in c["last_sem"]) + "\n")
            bits = c["depth_sum"].view(np.uint32)
            for l in range(16):
                f.write("%d %d %d %d\n" % (c["cnt"][l], c["bcnt"][l], c["sfcnt"][l], bits[l]))
            f.write(" ".join(str(v) for v in c["hist"].ravel()) + "\n")
