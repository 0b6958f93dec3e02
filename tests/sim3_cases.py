"""Generators of the Sim3Solver and SearchBySim3 test problems (fixed seeds): KITTI intrinsics,
points 6-30 m ahead of camera 1, a known similarity (s, R, t) with X1 = s R X2 + t, per-point noise
proportional to depth, a share of gross outliers, octaves 0..7."""
import numpy as np

from orb_ref_py import KP_DTYPE

f32 = np.float32
K_KITTI = (721.5377, 721.5377, 609.5593, 172.8540)
W, H = 1242, 375
NLEVELS = 8


def orb_scales(nlevels=NLEVELS, factor=1.2):
    """ORBextractor's mvScaleFactor / mvLevelSigma2 (float products, ORBextractor.cc:420-430)."""
    s = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        s[i] = f32(s[i - 1] * f32(factor))
    return s, (s * s).astype(f32)


def rot(axis, ang):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def points_ahead(rng, n, K=K_KITTI, margin=40.0):
    """n points 6-30 m ahead whose projection lies inside the image by `margin` pixels."""
    fx, fy, cx, cy = K
    z = rng.uniform(6.0, 30.0, n)
    u = rng.uniform(margin, W - margin, n)
    v = rng.uniform(margin, H - margin, n)
    return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)


def true_sim3(rng, fix_scale):
    s = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    R = rot(rng.normal(size=3), float(rng.uniform(0.02, 0.25)))
    t = rng.uniform(-0.6, 0.6, 3)
    return s, R, t


def solver_problem(seed, n, outlier_frac, noise, fix_scale, min_inliers=20, K1=K_KITTI,
                   K2=K_KITTI):
    """A Sim3Solver problem dict (Context.sim3solver_iterate's) with its truth: s, R, t and the
    inlier flags.  noise: standard deviation of the 3D noise in pixels at the point's depth."""
    rng = np.random.default_rng(seed)
    s, R, t = true_sim3(rng, fix_scale)
    X1 = points_ahead(rng, n, K1)
    X2 = ((X1 - t) @ R) / s  # R^T (X1 - t) / s
    fx = K1[0]
    X1n = X1 + rng.normal(size=(n, 3)) * (noise * X1[:, 2:3] / fx)
    X2n = X2 + rng.normal(size=(n, 3)) * (noise * X2[:, 2:3] / fx)
    inl = np.ones(n, bool)
    n_out = int(round(outlier_frac * n))
    if n_out:
        bad = rng.choice(n, n_out, replace=False)
        X2n[bad] = points_ahead(rng, n_out, K2)
        inl[bad] = False
    _, sigma2 = orb_scales()
    o1 = rng.integers(0, NLEVELS, n)
    o2 = np.clip(o1 + rng.integers(-1, 2, n), 0, NLEVELS - 1)
    return dict(X1=X1n.astype(f32), X2=X2n.astype(f32), sigma2_1=sigma2[o1], sigma2_2=sigma2[o2],
                K1=K1, K2=K2, fix_scale=fix_scale, probability=0.99,
                min_inliers=min_inliers, max_iterations=300,
                truth=dict(s=s, R=R, t=t, inliers=inl))


def draws(seed, n, iters):
    """DUtils::Random::RandomInt(0, n - 1 - j), j = 0..2, for `iters` iterations."""
    rng = np.random.default_rng(seed)
    out = np.zeros((iters, 3), np.int32)
    for j in range(3):
        out[:, j] = rng.integers(0, max(n - j, 1), iters)
    return out


# ------------------------------------------------------------------------------- SearchBySim3
def _flip(rng, desc, nbits):
    d = np.unpackbits(desc)
    d[rng.choice(256, nbits, replace=False)] ^= 1
    return np.packbits(d)


def _project(p, K=K_KITTI):
    fx, fy, cx, cy = K
    return np.stack([fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy], 1)


def keyframe_pair(seed, n_mutual, n_only=40, n_empty=40, s12=1.0, pix_noise=0.3, K=K_KITTI):
    """Two keyframes that see n_mutual common points under a known similarity (p1 = s12 R12 p2 +
    t12 between the camera frames), each with n_only points of its own and n_empty keys without a
    point.  The common points hold slots 0..n_mutual-1 of both keyframes, in a different order in
    keyframe 2 (pair[i1] = its key there).  Octaves and distance ranges are set so that every
    common point predicts, in the other keyframe, the octave of the key that observes it there.
    Returns (kf1, kf2, sim3, pair) with the keyframes as Context.search_by_sim3 takes them."""
    rng = np.random.default_rng(seed)
    R12 = rot(rng.normal(size=3), float(rng.uniform(0.03, 0.12)))
    t12 = rng.uniform(-0.5, 0.5, 3)
    log12 = np.log(1.2)
    P1, P2, O1, O2 = [], [], [], []
    while len(P1) < n_mutual:
        p1 = points_ahead(rng, 1, K)[0]
        p2 = (R12.T @ (p1 - t12)) / s12
        if p2[2] < 4.0:
            continue
        uv = _project(p2[None], K)[0]
        if not (40 <= uv[0] < W - 40 and 40 <= uv[1] < H - 40):
            continue
        delta = np.log(np.linalg.norm(p1) / np.linalg.norm(p2)) / log12
        m = int(np.rint(delta))
        o1 = int(rng.integers(1, 7))
        o2 = o1 + m
        if abs(delta - m) > 0.35 or not 1 <= o2 <= 6:
            continue
        P1.append(p1)
        P2.append(p2)
        O1.append(o1)
        O2.append(o2)
    P1, P2 = np.array(P1), np.array(P2)
    order2 = rng.permutation(n_mutual)  # slot of common point j in keyframe 2
    poses = []
    for _ in range(2):
        Rcw = rot(rng.normal(size=3), float(rng.uniform(0.1, 0.6)))
        tcw = rng.uniform(-3, 3, 3)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = Rcw, tcw
        poses.append(T.astype(f32))
    desc_pt = rng.integers(0, 256, (n_mutual, 32), dtype=np.uint8)
    kfs = []
    for side, (P, O) in enumerate(((P1, O1), (P2, O2))):
        n = n_mutual + n_only + n_empty
        own = points_ahead(rng, n_only, K)
        pc = np.concatenate([P, own, points_ahead(rng, n_empty, K)])
        octs = np.concatenate([np.array(O), rng.integers(1, 7, n_only + n_empty)])
        uv = _project(pc, K) + rng.normal(size=(n, 2)) * pix_noise
        uv[:, 0] = np.clip(uv[:, 0], 1, W - 2)
        uv[:, 1] = np.clip(uv[:, 1], 1, H - 2)
        slot = np.arange(n)
        if side == 1:
            slot[:n_mutual] = order2
        kps = np.zeros(n, KP_DTYPE)
        Xw = np.zeros((n, 3), f32)
        min_d, max_d = np.ones(n, f32), np.ones(n, f32)
        desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        pdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        skip = np.zeros(n, np.uint8)
        T = poses[side].astype(np.float64)
        for j in range(n):
            i = slot[j]
            kps["x"][i], kps["y"][i] = uv[j]
            kps["octave"][i] = octs[j]
            kps["size"][i] = 31.0
            d = np.linalg.norm(pc[j])
            max_d[i] = d * 1.2 ** (octs[j] - 0.5)
            min_d[i] = max_d[i] / 1.2 ** (NLEVELS - 1)
            Xw[i] = T[:3, :3].T @ (pc[j] - T[:3, 3])
            if j < n_mutual:  # the point's descriptor near both of its keys'
                pdesc[i] = _flip(rng, desc_pt[j], 6)
                desc[i] = _flip(rng, desc_pt[j], 10)
            elif j < n_mutual + n_only:
                desc[i] = _flip(rng, pdesc[i], 10)
            else:
                skip[i] = 1
        kfs.append(dict(kps=kps, desc=desc, depth=np.zeros((H, W), f32), Tcw=poses[side],
                        Xw=Xw, min_dist=min_d, max_dist=max_d, pdesc=pdesc, skip=skip))
    pair = order2.astype(np.int32)
    return kfs[0], kfs[1], dict(s=f32(s12), R=R12.astype(f32), t=t12.astype(f32)), pair


def add_twin_key(kf_src, i, kf_dst, k, dx, rng):
    """Append to kf_dst a key without a point, dx pixels beside key k, at the same octave and at
    the same Hamming distance from point i of kf_src as key k's descriptor.  Returns its index."""
    d0 = int(np.unpackbits(kf_src["pdesc"][i] ^ kf_dst["desc"][k]).sum())
    nd = np.unpackbits(kf_src["pdesc"][i])
    nd[rng.choice(256, d0, replace=False)] ^= 1
    new = kf_dst["kps"][k:k + 1].copy()
    new["x"] += f32(dx)
    kf_dst["kps"] = np.concatenate([kf_dst["kps"], new])
    kf_dst["desc"] = np.concatenate([kf_dst["desc"], np.packbits(nd)[None]])
    for name in ("Xw", "min_dist", "max_dist", "pdesc"):
        kf_dst[name] = np.concatenate([kf_dst[name], kf_dst[name][:1]])
    kf_dst["skip"] = np.concatenate([kf_dst["skip"], np.ones(1, np.uint8)])
    return len(kf_dst["skip"]) - 1


def edge_case(seed, n_mutual, s12):
    """keyframe_pair with one common point per skip reason (behind camera 2, outside its image,
    outside the distance range, its key at a wrong octave, its key moved out of the window), keys
    at equal Hamming distance on both sides of two keys (different grid cells: one twin wins and
    breaks the agreement, the other loses), and prior matches of the three kinds.  Returns (kf1,
    kf2, sim3, matched12)."""
    kf1, kf2, sim3, pair = keyframe_pair(seed, n_mutual, s12=s12)
    rng = np.random.default_rng(seed + 1)
    kf1["Xw"][3] = world_point(kf1, into_camera1(sim3, [0.5, 0.2, -8.0]))
    kf1["Xw"][4] = world_point(kf1, into_camera1(sim3, [40.0, 0.0, 10.0]))
    kf1["max_dist"][5] *= f32(0.25)
    kf1["min_dist"][5] *= f32(0.25)
    kf2["kps"]["octave"][pair[6]] = 0 if kf2["kps"]["octave"][pair[6]] >= 3 else 7
    kf2["kps"]["x"][pair[8]] += f32(200.0 if kf2["kps"]["x"][pair[8]] < W / 2 else -200.0)
    twins = 0
    for i in range(40, n_mutual):
        kp = kf2["kps"][pair[i]]
        if kp["octave"] >= 3 and 60 < kp["x"] < W - 60:
            add_twin_key(kf1, i, kf2, int(pair[i]), -11.0 if twins % 2 == 0 else 11.0, rng)
            twins += 1
            if twins == 4:
                break
    matched = np.full(len(kf1["skip"]), -1, np.int32)
    matched[10:20] = pair[10:20]
    matched[20:30] = -2
    return kf1, kf2, sim3, matched


def copy_kf(kf):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kf.items()}


def world_point(kf, pc):
    """The world position that keyframe `kf` sees at camera-frame position pc."""
    T = kf["Tcw"].astype(np.float64)
    return (T[:3, :3].T @ (np.asarray(pc, np.float64) - T[:3, 3])).astype(f32)


def into_camera1(sim3, p2):
    return float(sim3["s"]) * sim3["R"].astype(np.float64) @ np.asarray(p2, np.float64) + \
        sim3["t"].astype(np.float64)
