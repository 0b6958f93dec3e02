"""The per-frame object front end restated in NumPy, written from the reference's own lines
(src/Tracking.cc:447-465, 487-578, 1389-1630, 4007-4093; src/Frame.cc:188-324, 1118-1152) and from
nothing else: not from multimot_track_amd/csrc/ and not from oracle/.  The kernels
(csrc/mmt_track.hip), the host decisions (csrc/mmt_objdecide.cpp) and the CPU oracle
(oracle/track_ref.cpp) are all compared with this file, so a misreading they share shows.

Floats are float32 wherever the reference computes in float, and every float32 operation is its
own rounding (no fused multiply-add).  Plain loops where the order matters.

Pins (places where the reference leaves the value open and the project chose one):
  * `int max` is uninitialised when the last frame has no object and bSecondFrame is false
    (Tracking.cc:1557-1568): the project starts the new labels at 1, and so does decide().
  * std::sort(sorted, sort_pair_int) on at most 15 pairs is libstdc++'s insertion sort, which never
    moves an element past one that compares equal: on equal counts std::map's ascending key order
    survives, and the smaller last label wins.
  * UnprojectStereoObject returns an empty cv::Mat at a depth <= 0 and the caller reads it
    (undefined): not restated, groups() asserts positive depths on the samples it unprojects.
  * The project keeps semantic labels in [0, 15]; groups() raises on a larger one.

One reading here does not come from the reference's lines, because the lines do not settle it:
how OpenCV evaluates `Rwl*x3Dc+twl` and `-Rlw.t()*tlw` on 3x3 and 3x1 float matrices.
unproject_world() takes each product as a cv::gemm that accumulates in double and rounds its
result to float, and the sum with twl as a float addition.  OpenCV may instead fold twl into one
gemm (one rounding of the double sum plus twl), or take a small-matrix path that accumulates in
float.  The kernel and the oracle share this reading; it stays unpinned.
"""
import numpy as np

F32 = np.float32


# ------------------------------------------------------------------ A2 (Tracking.cc:447-465)
def gray_depth(bgr, disp, bf):
    """cvtColor(CV_RGB2GRAY) on 8-bit data is OpenCV 3's fixed-point (R2Y, G2Y, B2Y) = (4899,
    9617, 1868), shift 14, rounded, with the first channel taken as R.
    depth: `float dp = imD.at<float>(i,j)/256.0; imD.at<float>(i,j) = mbf/dp;` -- the disparity as
    a float, divided in double, stored to a float, then a float division.  d = 0 gives inf."""
    c = np.asarray(bgr).astype(np.int64)
    gray = ((c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + (1 << 13)) >> 14)
    d = np.asarray(disp).astype(F32)
    dp = (d.astype(np.float64) / 256.0).astype(F32)
    with np.errstate(divide="ignore"):
        depth = F32(bf) / dp
    return gray.astype(np.uint8), depth.astype(F32)


# ------------------------------------------------------------------ B1 (Frame.cc:188-217)
def object_samples(depth, flow, mask):
    """Every 4th row and column, rows outer: keep where maskSEM != 0 && depth < 25 && depth > 0
    and j+flow_x < cols && j+flow_x > 0 && i+flow_y < rows && i+flow_y > 0 (int + float: float)."""
    H, W = depth.shape
    keys, corres, fl, dep, lab = [], [], [], [], []
    for i in range(0, H, 4):
        for j in range(0, W, 4):
            d = depth[i, j]
            if mask[i, j] != 0 and d < 25 and d > 0:
                fx, fy = F32(flow[i, j, 0]), F32(flow[i, j, 1])
                cx, cy = F32(j) + fx, F32(i) + fy
                if cx < F32(W) and cx > 0 and cy < F32(H) and cy > 0:
                    fl.append((fx, fy))
                    corres.append((cx, cy))
                    keys.append((j, i))
                    dep.append(d)
                    lab.append(mask[i, j])
    return dict(keys=np.array(keys, F32).reshape(-1, 2), corres=np.array(corres, F32).reshape(-1, 2),
                flow=np.array(fl, F32).reshape(-1, 2), depth=np.array(dep, F32),
                label=np.array(lab, np.int32), count=len(dep))


def object_samples_vec(depth, flow, mask):
    """object_samples vectorised (row-major order is NumPy's own), for full-size images."""
    H, W = depth.shape
    ii, jj = np.meshgrid(np.arange(0, H, 4), np.arange(0, W, 4), indexing="ij")
    ii, jj = ii.ravel(), jj.ravel()
    d, m = depth[ii, jj], mask[ii, jj]
    f = flow[ii, jj].astype(F32)
    cx, cy = jj.astype(F32) + f[:, 0], ii.astype(F32) + f[:, 1]
    keep = (m != 0) & (d < 25) & (d > 0) & (cx < F32(W)) & (cx > 0) & (cy < F32(H)) & (cy > 0)
    k = np.nonzero(keep)[0]
    return dict(keys=np.stack([jj[k], ii[k]], 1).astype(F32), corres=np.stack([cx[k], cy[k]], 1),
                flow=f[k], depth=d[k].astype(F32), label=m[k].astype(np.int32), count=len(k))


# ------------------------------------------------------------------ B2 (Frame.cc:228-324)
def static_samples(kps_xy, depth, flow, mask):
    """Per ORB key, in key order: x = (int)pt.x, y = (int)pt.y; dropped when maskSEM(y,x) != 0,
    when depth(y,x) > 40 || depth(y,x) <= 0, unless both flow components != 0, and unless
    pt.x+flow_x < cols && pt.y+flow_y < rows && pt.x < cols && pt.y < rows (no lower bound).
    mvSiftDepthTmp is -1 unless the depth at the truncated key is > 0."""
    H, W = depth.shape
    keys, corres, fl, dep = [], [], [], []
    for px, py in np.asarray(kps_xy, F32).reshape(-1, 2):
        x, y = int(px), int(py)  # float -> int truncates
        if mask[y, x] != 0:
            continue
        if depth[y, x] > 40 or depth[y, x] <= 0:
            continue
        fxe, fye = F32(flow[y, x, 0]), F32(flow[y, x, 1])
        if fxe != 0 and fye != 0:
            if px + fxe < F32(W) and py + fye < F32(H) and px < F32(W) and py < F32(H):
                keys.append((px, py))
                corres.append((px + fxe, py + fye))
                fl.append((fxe, fye))
    for px, py in keys:
        d = depth[int(py), int(px)]
        dep.append(d if d > 0 else F32(-1))
    return dict(keys=np.array(keys, F32).reshape(-1, 2), corres=np.array(corres, F32).reshape(-1, 2),
                flow=np.array(fl, F32).reshape(-1, 2), depth=np.array(dep, F32), count=len(dep))


# ------------------------------------------------------------------ B4 (Tracking.cc:487-578)
def c_round(x):
    """std::round: half away from zero (NaN stays NaN).  Exact: |x| + 0.5 in double."""
    x = np.asarray(x, np.float64)
    return np.copysign(np.floor(np.abs(x) + 0.5), x)


def handoff(last_corres, last_obj_corres, depth, mask):
    """mvSiftKeys = last mvCorres with depth -1 unless 0 < round(u) < cols, 0 < round(v) < rows and
    the depth there is > 0; mvObjKeys = last mvObjCorres with depth and label read there, or 0.1
    and 0 outside."""
    H, W = depth.shape
    sk = np.asarray(last_corres, F32).reshape(-1, 2)
    ok = np.asarray(last_obj_corres, F32).reshape(-1, 2)
    sd = np.full(len(sk), -1, F32)
    for i, (u, v) in enumerate(sk):
        ru, rv = c_round(u), c_round(v)
        if ru < W and ru > 0 and rv < H and rv > 0:
            d = depth[int(rv), int(ru)]
            if d > 0:
                sd[i] = d
    od = np.full(len(ok), -1, F32)
    ol = np.full(len(ok), -1, np.int32)
    for i, (u, v) in enumerate(ok):
        ru, rv = c_round(u), c_round(v)
        if ru < W and ru > 0 and rv < H and rv > 0:
            od[i] = depth[int(rv), int(ru)]
            ol[i] = mask[int(rv), int(ru)]
        else:
            od[i] = F32(0.1)
            ol[i] = 0
    return dict(skeys=sk.copy(), sdepth=sd, okeys=ok.copy(), odepth=od, olabel=ol, ns=len(sk),
                no=len(ok))


def handoff_vec(last_corres, last_obj_corres, depth, mask):
    """handoff vectorised, for full-size sample sets."""
    H, W = depth.shape

    def inside(k):
        with np.errstate(invalid="ignore"):
            ru, rv = c_round(k[:, 0]), c_round(k[:, 1])
            ok = (ru < W) & (ru > 0) & (rv < H) & (rv > 0)
        return ok, np.where(ok, ru, 0).astype(np.int64), np.where(ok, rv, 0).astype(np.int64)

    sk = np.asarray(last_corres, F32).reshape(-1, 2)
    okk = np.asarray(last_obj_corres, F32).reshape(-1, 2)
    a, ru, rv = inside(sk)
    d = depth[rv, ru]
    sd = np.where(a & (d > 0), d, F32(-1)).astype(F32)
    b, ru, rv = inside(okk)
    od = np.where(b, depth[rv, ru], F32(0.1)).astype(F32)
    ol = np.where(b, mask[rv, ru], 0).astype(np.int32)
    return dict(skeys=sk.copy(), sdepth=sd, okeys=okk.copy(), odepth=od, olabel=ol, ns=len(sk),
                no=len(okk))


# ------------------------------------------------------------------ B6 (Frame.cc:1118-1152)
def unproject_world(Tcw, K, keys, z):
    """UnprojectStereoObject(i, 0) for many samples: x = (u-cx)*z*invfx, y = (v-cy)*z*invfy in
    float (invfx = 1.0f/fx); Rwl = Rlw.t(); twl = -Rlw.t()*tlw, a float matrix of its own;
    Rwl*x3Dc + twl.  cv::gemm on float matrices accumulates each output element in double and
    rounds it to float; the sum with twl is a float addition."""
    fx, fy, cx, cy = (F32(v) for v in K)
    T = np.asarray(Tcw, F32).reshape(4, 4)
    keys = np.asarray(keys, F32).reshape(-1, 2)
    z = np.asarray(z, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (keys[:, 0] - cx) * z * (F32(1.0) / fx)
        y = (keys[:, 1] - cy) * z * (F32(1.0) / fy)
        xc = np.stack([x, y, z], 1).astype(np.float64)
        R = T[:3, :3].astype(np.float64)
        t = T[:3, 3].astype(np.float64)
        out = np.zeros((len(z), 3), F32)
        for r in range(3):
            s = 0.0
            p = np.zeros(len(z), np.float64)
            for k in range(3):  # Rwl[r][k] = Rlw[k][r]
                s = s + R[k, r] * t[k]
                p = p + R[k, r] * xc[:, k]
            out[:, r] = p.astype(F32) + F32(-s)
    return out


def scene_flow_norm(xc, xp):
    """flow3d = x3D_c - x3D_p (float); sf_norm = std::sqrt(flow.x*flow.x + flow.z*flow.z): the y
    component is not part of it (Tracking.cc:1475)."""
    with np.errstate(invalid="ignore", over="ignore"):
        f0 = (xc[:, 0] - xp[:, 0]).astype(F32)
        f2 = (xc[:, 2] - xp[:, 2]).astype(F32)
        return np.sqrt((f0 * f0 + f2 * f2).astype(F32)).astype(F32)


# ------------------------------------------------------- B6 + B7 statistics (Tracking.cc:1396-1536)
def groups(cur_keys, cur_depth, cur_label, last_keys, last_depth, last_label, Tcur, Tlast, K, W, H):
    """GetSceneFlowObj marks a sample -1 when its current or its last semantic label is <= 0 (the
    others keep vObjLabel's initial -2); Posi[label] lists the unmarked samples in index order.
    Per label: cnt, the boundary count (v<25 || v>rows-25 || u<50 || u>cols-50), the count of
    sf_norm < 0.12f, obj_center_depth as a sequential float sum in Posi order, and the last-frame
    labels of its samples (dups)."""
    ck = np.asarray(cur_keys, F32).reshape(-1, 2)
    cd = np.asarray(cur_depth, F32)
    cl = np.asarray(cur_label, np.int32)
    ll = np.asarray(last_label, np.int32)
    n = len(cd)
    if n and max(cl.max(), ll.max()) > 15:
        raise ValueError("semantic label above 15")
    obj_label = np.where((cl <= 0) | (ll <= 0), -1, -2).astype(np.int32)
    live = np.nonzero(obj_label != -1)[0]
    assert (cd[live] > 0).all() and (np.asarray(last_depth, F32)[live] > 0).all(), \
        "depth <= 0 on an unprojected sample: undefined in the reference"
    sf = np.full(n, np.nan, F32)
    xp = unproject_world(Tlast, K, np.asarray(last_keys, F32).reshape(-1, 2)[live],
                         np.asarray(last_depth, F32)[live])
    xc = unproject_world(Tcur, K, ck[live], cd[live])
    sf[live] = scene_flow_norm(xc, xp)
    members = [np.zeros(0, np.int32) for _ in range(16)]
    cnt, bcnt, sfcnt = (np.zeros(16, np.int32) for _ in range(3))
    depth_sum = np.zeros(16, F32)
    hist = np.zeros((16, 16), np.int32)
    for l in range(1, 16):
        posi = live[cl[live] == l].astype(np.int32)
        members[l] = posi
        cnt[l] = len(posi)
        u, v = ck[posi, 0], ck[posi, 1]
        bcnt[l] = int(((v < 25) | (v > (H - 25)) | (u < 50) | (u > (W - 50))).sum())
        sfcnt[l] = int((sf[posi] < F32(0.12)).sum())
        if len(posi):
            with np.errstate(over="ignore", invalid="ignore"):
                depth_sum[l] = np.add.accumulate(cd[posi], dtype=F32)[-1]  # sequential, in order
        for k in ll[posi]:
            hist[l, k] += 1
    return dict(obj_label=obj_label, members=members, cnt=cnt, bcnt=bcnt, sfcnt=sfcnt,
                depth_sum=depth_sum, hist=hist, sf=sf)


# ------------------------------------------------- B7 decisions + B8 (Tracking.cc:1424-1630)
def decide(cnt, bcnt, sfcnt, depth_sum, hist, bSecond, last_mod_label, last_sem_position):
    """Labels ascending (UniLab is sorted).  A label is dropped when count/size > 0.5f (float
    count over a size_t: a float division), unless size > 100, when sf_count/size > 0.3f, or when
    obj_center_depth/size > 25.0.  An empty Posi gives 0/0 = NaN, which is not > 0.5, and then
    fails size > 100.  Returns (SemPosNew, LabId)."""
    kept = []
    for l in range(1, 16):
        size = int(cnt[l])
        with np.errstate(invalid="ignore", divide="ignore"):
            if F32(bcnt[l]) / F32(size) > F32(0.5):
                continue
            if not size > 100:
                continue
            if F32(sfcnt[l]) / F32(size) > F32(0.3):
                continue
            if float(F32(depth_sum[l]) / F32(size)) > 25.0:
                continue
        kept.append(l)
    if bSecond:
        mx = 1
    elif len(last_mod_label) > 0:
        mx = max(last_mod_label) + 1
    else:
        mx = 1  # uninitialised in the reference: the project's pin
    lab_id = []
    for l in kept:
        dups = [(k, int(hist[l][k])) for k in range(16) if hist[l][k] > 0]  # std::map: ascending
        dups.sort(key=lambda kv: -kv[1])  # stable, as the insertion sort of <= 15 pairs is
        new_lab = dups[0][0]
        if bSecond:
            lab_id.append(mx)
            mx += 1
            continue
        for k, s in enumerate(last_sem_position):
            if s == new_lab:
                lab_id.append(last_mod_label[k])
                break
        else:
            lab_id.append(mx)
            mx += 1
    return kept, lab_id
