"""GPU parity of the tracking half of the hot path
against the CPU oracle: single solves through the probe entry points, then whole kitti_sample
sequences through mmt_track_rgbd / mmt_track_rgbd_chunk_device.

Tolerance (north_star): SE(3) poses within 1e-4 (max abs over the 4x4 entries); integer
outputs (counts, labels, iterations, inlier sets) exact; the object centroid of the speed
evaluation (ObjCentre3D_pre, world metres) within 1e-3."""
import numpy as np
import pytest

from synth_problems import K_KITTI, flow_problem, pnp_problem

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-4
CENTRE_TOL = 1e-3  # metres; an evaluation output (the object-speed estimate), not a pose


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(nfeatures=2000, max_batch=8))
    yield c
    c.close()


@pytest.mark.parametrize("seed,n,out,ego", [(0, 400, 0.0, True), (1, 600, 0.1, True),
                                             (2, 1500, 0.2, True), (3, 300, 0.15, False),
                                             (4, 3000, 0.3, False), (5, 3, 0.0, False),
                                             (6, 37, 0.3, True)])
def test_flow_solve_matches_oracle(ctx, oracle_mod, seed, n, out, ego):
    obs, flow, depth, Tl, init, _ = flow_problem(seed, n, outlier_frac=out)
    args = (0.04, 0.3, 100) if ego else (0.01, 0.5, 200)
    rc, pose_o, st_o = oracle_mod.flow_solve(obs, flow, depth, Tl, init, *args, K_KITTI)
    status, pose_g, st_g = ctx.flow_solve(obs, flow, depth, Tl, init, *args, K_KITTI)
    assert status == rc
    if rc == 0:
        assert np.abs(pose_g - pose_o).max() < POSE_TOL
    assert st_g["inliers"] == st_o["inliers"]
    if n >= 10:
        # a 3-edge problem is barely constrained: the LM creeps for ~75 iterations and the
        # stop test flips on last-bit differences of the reduction order (pose still agrees)
        assert st_g["iterations"] == st_o["iterations"]


@pytest.mark.parametrize("seed,n,noise,ego", [(24, 200, 0.0, True), (24, 200, 0.02, False),
                                               (3, 40, 0.0, False), (24, 40, 0.02, True)])
def test_flow_solve_rejection_chains_bit_exact(ctx, oracle_mod, seed, n, noise, ego,
                                               monkeypatch):
    """The lambda candidate table of the flow LM: after a rejection on a system without
    Huber-active edges the next trials take their increment and pose from candidates solved in
    advance for lambda * ni, ...  These problems (large motion, little noise) reject several
    trials in a row on clean systems (the oracle counts them), so candidates 1-3 are used; the
    solve must be bit-identical to one that solves every trial for its own lambda
    (MMT_LM_MAX_CAND=1), and agree with the oracle within 1e-4."""
    obs, flow, depth, Tl, init, _ = flow_problem(seed, n, outlier_frac=0.0, pix_noise=noise,
                                                 motion=0.3)
    args = (0.04, 0.3, 100) if ego else (0.01, 0.5, 200)
    rc, pose_o, st_o = oracle_mod.flow_solve(obs, flow, depth, Tl, init, *args, K_KITTI)
    assert st_o["clean_rejections"] >= 4 and st_o["max_reject_run"] >= 4, st_o
    status4, pose4, st4 = ctx.flow_solve(obs, flow, depth, Tl, init, *args, K_KITTI)
    monkeypatch.setenv("MMT_LM_MAX_CAND", "1")
    status1, pose1, st1 = ctx.flow_solve(obs, flow, depth, Tl, init, *args, K_KITTI)
    assert status4 == status1 == rc == 0
    assert np.array_equal(pose4, pose1) and st4 == st1
    assert np.abs(pose4 - pose_o).max() < POSE_TOL
    assert st4["inliers"] == st_o["inliers"]


@pytest.mark.parametrize("seed,n,out,ego,groups", [
    (2, 1500, 0.2, True, "0"), (2, 1500, 0.2, True, "2"), (2, 1500, 0.2, True, "8"),
    (1, 600, 0.1, True, "3"), (4, 3000, 0.3, False, "5"), (6, 37, 0.3, True, "8"),
    (9, 5, 0.0, True, "8"), (10, 1700, 0.05, True, "7")])
def test_flow_solve_split_matches_oracle(ctx, oracle_mod, seed, n, out, ego, groups, monkeypatch):
    """The large ego solve split over workgroups that exchange their sums at every reduction
    (launch_flow_lm_split): any group count, including slices of no edges (n=5 over 8), agrees
    with the oracle as the whole solve does (MMT_LM_SPLIT=0)."""
    monkeypatch.setenv("MMT_LM_SPLIT", groups)
    obs, flow, depth, Tl, init, _ = flow_problem(seed, n, outlier_frac=out)
    args = (0.04, 0.3, 100) if ego else (0.01, 0.5, 200)
    rc, pose_o, st_o = oracle_mod.flow_solve(obs, flow, depth, Tl, init, *args, K_KITTI)
    status, pose_g, st_g = ctx.flow_solve(obs, flow, depth, Tl, init, *args, K_KITTI)
    assert status == rc == 0
    assert np.abs(pose_g - pose_o).max() < POSE_TOL
    assert st_g["inliers"] == st_o["inliers"]
    if n >= 10:
        assert st_g["iterations"] == st_o["iterations"]


@pytest.mark.parametrize("seed,n,noise,ego", [(24, 1200, 0.0, True), (24, 900, 0.02, False)])
def test_flow_solve_split_rejection_chains_bit_exact(ctx, oracle_mod, seed, n, noise, ego,
                                                     monkeypatch):
    """The split solve's lambda candidates: bit-identical to solving every trial for its own
    lambda, as in the whole solve."""
    monkeypatch.setenv("MMT_LM_SPLIT", "4")
    obs, flow, depth, Tl, init, _ = flow_problem(seed, n, outlier_frac=0.0, pix_noise=noise,
                                                 motion=0.3)
    args = (0.04, 0.3, 100) if ego else (0.01, 0.5, 200)
    rc, pose_o, st_o = oracle_mod.flow_solve(obs, flow, depth, Tl, init, *args, K_KITTI)
    status4, pose4, st4 = ctx.flow_solve(obs, flow, depth, Tl, init, *args, K_KITTI)
    monkeypatch.setenv("MMT_LM_MAX_CAND", "1")
    status1, pose1, st1 = ctx.flow_solve(obs, flow, depth, Tl, init, *args, K_KITTI)
    assert status4 == status1 == rc == 0
    assert np.array_equal(pose4, pose1) and st4 == st1
    assert np.abs(pose4 - pose_o).max() < POSE_TOL
    assert st4["inliers"] == st_o["inliers"]


def test_flow_solve_too_few_edges(ctx):
    obs, flow, depth, Tl, init, _ = flow_problem(8, 2)
    status, _, st = ctx.flow_solve(obs, flow, depth, Tl, init, 0.04, 0.3, 100, K_KITTI)
    assert status == 1 and st["iterations"] == 0


@pytest.mark.parametrize("seed,n,out", [(0, 200, 0.3), (1, 1000, 0.5), (2, 5, 0.0),
                                        (3, 64, 0.2), (4, 3000, 0.6), (5, 130, 0.9)])
def test_pnp_ransac_matches_oracle(ctx, oracle_mod, seed, n, out):
    p3, p2, _ = pnp_problem(seed, n, outlier_frac=out, pix_noise=0.05)
    rc, R_o, t_o, inl_o, info_o = oracle_mod.pnp_ransac(p3, p2, K_KITTI)
    R_g, t_g, inl_g, info_g = ctx.pnp_ransac(p3, p2, K_KITTI)
    assert info_g["iterations"] == info_o["iterations"]
    assert info_g["best_iter"] == info_o["best_iter"]
    assert sorted(inl_g.tolist()) == sorted(inl_o.tolist())
    if rc == 0:
        assert np.abs(R_g - R_o).max() < POSE_TOL
        assert np.abs(t_g - t_o).max() < POSE_TOL


def _compare_frame(g, o, i):
    """Every integer output exact (frame counts, ego LM stats, the map branch's matches,
    inliers, keyframe decisions and map sizes, each object's labels and solve statistics), every
    pose within 1e-4 (the frame's, the map branch's, each object's), centroids within 1e-3 m (NaN
    on both sides for a solve without points): oracle/compare.py."""
    from oracle import compare
    p, c, bad = compare.compare_frame(g, o)[:3]
    assert not bad, (i, bad)
    assert p < POSE_TOL, (i, p, g["Tcw"], o["Tcw"])
    assert c < CENTRE_TOL, (i, c)


def test_track_kitti_sequence_matches_oracle(ctx, oracle_mod, kitti_frames):
    ctx.reset()
    tr = oracle_mod.Tracker(1242, 375, K_KITTI, 387.5744, 0, 2000)
    for i, f in enumerate(kitti_frames):
        o = tr.track(f["bgr"], f["disp"], f["flow"], f["sem"])
        g = ctx.track(f["bgr"], f["disp"], f["flow"], f["sem"])
        _compare_frame(g, o, i)


def test_track_chunk_device_equals_per_frame(ctx, kitti_frames):
    import torch
    ctx.reset()
    per = [ctx.track(f["bgr"], f["disp"], f["flow"], f["sem"]) for f in kitti_frames]
    ctx.reset()
    dev = torch.device("cuda:0")
    bgr = torch.from_numpy(np.stack([f["bgr"] for f in kitti_frames])).to(dev)
    disp = torch.from_numpy(np.stack([f["disp"].view(np.int16) for f in kitti_frames])).to(dev)
    flow = torch.from_numpy(np.stack([f["flow"] for f in kitti_frames])).to(dev)
    mask = torch.from_numpy(np.stack([f["sem"] for f in kitti_frames])).to(dev)
    torch.cuda.synchronize()
    got = ctx.track_chunk_device(bgr[:3], disp[:3], flow[:3], mask[:3])
    got += ctx.track_chunk_device(bgr[3:], disp[3:], flow[3:], mask[3:])
    for i, (a, b) in enumerate(zip(got, per)):
        assert np.array_equal(a["Tcw"], b["Tcw"]), i
        assert [o["label"] for o in a["objects"]] == [o["label"] for o in b["objects"]]
        for x, y in zip(a["objects"], b["objects"]):
            assert np.array_equal(x["motion"], y["motion"])


def test_track_static_scene_without_objects(ctx, oracle_mod, kitti_frames):
    """No semantic labels: ego-only tracking (C2-style input), objects list stays empty."""
    ctx.reset()
    tr = oracle_mod.Tracker(1242, 375, K_KITTI, 387.5744, 0, 2000)
    for i, f in enumerate(kitti_frames[:3]):
        z = np.zeros_like(f["sem"])
        o = tr.track(f["bgr"], f["disp"], f["flow"], z)
        g = ctx.track(f["bgr"], f["disp"], f["flow"], z)
        _compare_frame(g, o, i)
        assert g["objects"] == []


def _synthetic_parity(w, h, nfeat, nobj, nframes, seed):
    import multimot_track_amd as M
    from multimot_track_amd import scene
    from oracle import oracle as O
    frames = scene.to_numpy_frames(scene.kitti_like_sequence(nframes, w, h, n_objects=nobj,
                                                             seed=seed))
    c = M.Context(M.kitti03_config(w, h, nfeat, max_batch=4))
    tr = O.Tracker(w, h, K_KITTI, 387.5744, 0, nfeat)
    n_obj = 0
    try:
        for i, f in enumerate(frames):
            o = tr.track(f["bgr"], f["disp"], f["flow"], f["sem"])
            g = c.track(f["bgr"], f["disp"], f["flow"], f["sem"])
            _compare_frame(g, o, i)
            n_obj = max(n_obj, len(g["objects"]))
    finally:
        c.close()
    return n_obj


def test_track_synthetic_c3_matches_oracle(oracle_mod):
    """BASELINE C3 geometry: ego + 3 moving boxes, 2000 features."""
    assert _synthetic_parity(1242, 375, 2000, 3, 8, 1003) == 3


def test_track_synthetic_c2_ego_only_matches_oracle(oracle_mod):
    assert _synthetic_parity(1242, 375, 2000, 0, 5, 1005) == 0


def test_track_synthetic_c5_1080p_matches_oracle(oracle_mod):
    """BASELINE C5 geometry: 1920x1080, 8000 features, 8 moving boxes.  Eight car-sized boxes
    in the scene's 15 m street occlude each other and the B7 filters (fewer than 100 samples,
    beyond 25 m) drop some; test_track_c5_eight_motions_long_matches_oracle below tracks eight
    object motions in every frame."""
    assert _synthetic_parity(1920, 1080, 8000, 8, 4, 2000) >= 4


def _long_parity(oracle_mod, w, h, nfeat, n, seed, objects, lanes=None, parts=1, chunk=32):
    """n frames through the bench's entry point (chunks of `chunk` frames) against the oracle
    frame by frame; objects split into `parts` rigid column bands (split_labels)."""
    import torch
    import multimot_track_amd as M
    from multimot_track_amd import scene
    from oracle import compare
    seq = scene.kitti_like_sequence(n, w, h, n_objects=objects, seed=seed, device="cuda:0",
                                    lanes=lanes)
    frames = scene.to_numpy_frames(seq)
    if parts > 1:
        for f in frames:
            f["sem"] = split_labels(f["sem"], parts)
    dev = torch.device("cuda:0")
    T = lambda k: torch.from_numpy(np.stack([f[k] for f in frames]))  # noqa: E731
    bgr, disp = T("bgr").to(dev), T("disp").view(torch.int16).to(dev)
    flow, mask = T("flow").to(dev), T("sem").to(dev)
    ctx = M.Context(M.kitti03_config(w, h, nfeat, max_batch=chunk))
    got = []
    try:
        for s0 in range(0, n, chunk):
            sl = slice(s0, min(n, s0 + chunk))
            got += ctx.track_chunk_device(bgr[sl], disp[sl], flow[sl], mask[sl])
    finally:
        ctx.close()
    tr = oracle_mod.Tracker(w, h, K_KITTI, 387.5744, 0, nfeat)
    ora = [tr.track(f["bgr"], f["disp"], f["flow"], f["sem"]) for f in frames]
    rec = compare.parity_record(got, ora)
    print(rec)
    if rec["first_divergent_frame"] is not None:  # the frames up to the divergence
        k = rec["first_divergent_frame"]
        print("up to frame", k, compare.parity_record(got[:k], ora[:k]))
        print("gpu", got[k]["objects"], "\noracle", ora[k]["objects"])
    assert rec["first_divergent_frame"] is None, rec
    assert rec["lm_stop_flips"] <= compare.lm_flip_budget(rec["frames"]), rec
    return got, rec


def test_track_c5_eight_motions_long_matches_oracle(oracle_mod):
    """C5's eight object motions at 1920x1080 with 8000 features over 100 frames: two boxes,
    each split into four rigid column bands with labels of their own (eight rigid moving
    objects), every one solved in every tracked frame and every frame within the bar."""
    got, rec = _long_parity(oracle_mod, 1920, 1080, 8000, 100, 2000, 2,
                            lanes=[(-3.0, 12.0), (3.4, 9.0)], parts=4)
    assert all(len(g["objects"]) == 8 for g in got[1:])
    assert rec["frames"] == 100


@pytest.mark.parametrize("w,h,seed", [(1241, 376, 1000), (1226, 370, 1005)])
def test_track_c4_sizes_long_matches_oracle(oracle_mod, w, h, seed):
    """BASELINE C4 geometries (KITTI 00 at 1241x376, 05/07 at 1226x370), 4000 features, ego + 3
    moving boxes, over 100 frames (keyframes, local BA and fusion; the cull branch is covered by
    test_gpu_localmap.py::test_keyframe_culling_and_reparenting_match_oracle)."""
    got, rec = _long_parity(oracle_mod, w, h, 4000, 100, seed, 3)
    assert rec["frames"] == 100 and got[-1]["n_keyframes"] > 2


def test_track_c4_400_frames_matches_oracle(oracle_mod):
    """C4 depth: KITTI 00's geometry over 400 frames (about a tenth of a real C4 sequence),
    tracked on the map in every frame, every frame within the bar."""
    got, rec = _long_parity(oracle_mod, 1241, 376, 4000, 400, 1000, 3, chunk=64)
    assert rec["frames"] == 400 and got[-1]["n_keyframes"] > 10
    assert all(g["map_state"] == 1 for g in got)


def test_track_c5_eight_motions_250_frames_matches_oracle(oracle_mod):
    """C5 depth: the eight object motions at 1920x1080 and 8000 features over 250 frames."""
    got, rec = _long_parity(oracle_mod, 1920, 1080, 8000, 250, 2000, 2,
                            lanes=[(-3.0, 12.0), (3.4, 9.0)], parts=4)
    assert rec["frames"] == 250
    assert sum(len(g["objects"]) == 8 for g in got[1:]) >= 240
    assert all(g["map_state"] == 1 for g in got)


@pytest.mark.parametrize("seed,n,out,mono", [(0, 400, 0.15, 0.2), (1, 1500, 0.2, 0.1),
                                             (2, 60, 0.3, 0.5), (3, 8, 0.0, 0.3),
                                             (4, 2048, 0.1, 0.0), (5, 300, 0.0, 1.0),
                                             (6, 2049, 0.1, 0.1), (7, 7000, 0.25, 0.2)])
def test_pose_optimization_matches_oracle(ctx, oracle_mod, seed, n, out, mono):
    """D1 (Optimizer::PoseOptimization): pose within 1e-4, mvbOutlier and the inlier count
    exact, for mixed mono/stereo edges, outliers, the one-round (< 10 edges) case, the 2048
    edges the register kernels hold and the global-scratch path beyond (C4/C5 frames
    carry up to 8000 keys)."""
    from synth_problems import pose_opt_problem
    Xw, obs, s2, init, _ = pose_opt_problem(seed, n, outlier_frac=out, mono_frac=mono)
    n_o, pose_o, outl_o = oracle_mod.pose_optimization(Xw, obs, s2, init, K_KITTI, 387.5744)
    n_g, pose_g, outl_g = ctx.pose_optimization(Xw, obs, s2, init, K_KITTI, 387.5744)
    assert np.abs(pose_g - pose_o).max() < POSE_TOL
    assert n_g == n_o
    assert np.array_equal(outl_g, outl_o)


def test_pose_optimization_too_few_edges(ctx):
    from synth_problems import pose_opt_problem
    Xw, obs, s2, init, _ = pose_opt_problem(9, 2)
    n_g, pose_g, outl_g = ctx.pose_optimization(Xw, obs, s2, init, K_KITTI, 387.5744)
    assert n_g == 0 and np.array_equal(pose_g, init) and not outl_g.any()


@pytest.mark.parametrize("w,h,seed", [(1241, 376, 1000), (1226, 370, 1005)])
def test_track_synthetic_c4_sizes_matches_oracle(oracle_mod, w, h, seed):
    """BASELINE C4 geometries (KITTI 00 at 1241x376, 05/07 at 1226x370), 4000 features,
    ego + 3 moving boxes."""
    assert _synthetic_parity(w, h, 4000, 3, 5, seed) >= 1


def test_track_reports_orb_device_flags(kitti_frames):
    """TrackRGBD checks the ORB device error word at its host sync: a tripped octree guard is an
    error return, not a frame tracked on truncated keypoints."""
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(nfeatures=2000))
    f = kitti_frames[0]
    c.debug_orb_raise(2)
    with pytest.raises(M.MmtError, match="octree-node-capacity"):
        c.track(f["bgr"], f["disp"], f["flow"], f["sem"])
    c.reset()
    r = c.track(f["bgr"], f["disp"], f["flow"], f["sem"])
    assert r["n_keys"] > 500
    c.close()


def test_track_continues_after_device_error(oracle_mod, kitti_frames):
    """A call whose ORB trips a device guard tracks none of its frames and leaves the context as
    the previous call left it: tracking the sequence on without mmt_reset matches the oracle
    tracking it with the failed frame absent."""
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(nfeatures=2000))
    tr = oracle_mod.Tracker(1242, 375, K_KITTI, 387.5744, 0, 2000)
    try:
        for i, f in enumerate(kitti_frames):
            if i == 2:
                c.debug_orb_raise(2)
                with pytest.raises(M.MmtError, match="octree-node-capacity"):
                    c.track(f["bgr"], f["disp"], f["flow"], f["sem"])
            g = c.track(f["bgr"], f["disp"], f["flow"], f["sem"])
            o = tr.track(f["bgr"], f["disp"], f["flow"], f["sem"])
            _compare_frame(g, o, i)
    finally:
        c.close()


def split_labels(sem, parts=5):
    """Each box's label split into `parts` column bands (rigid parts of one box are rigid
    objects of their own): the default 3-box street gives 10 dynamic objects."""
    out = np.zeros_like(sem)
    for L in (1, 2, 3):
        m = sem == L
        if not m.any():
            continue
        cols = np.nonzero(m.any(0))[0]
        u0, w = cols.min(), cols.max() - cols.min() + 1
        q = np.minimum(parts - 1, (np.arange(sem.shape[1]) - u0) * parts // w)
        out = np.where(m, 1 + (L - 1) * parts + q[None, :], out)
    return out.astype(np.int32)


def test_track_ten_objects_matches_oracle(ctx, oracle_mod):
    """More than 8 dynamic objects per frame (round 2 silently dropped objects 9+): 10 objects,
    one of them with an empty solve (its centroid is NaN, as the reference's 0 / 0)."""
    from multimot_track_amd import scene
    from oracle import compare
    seq = scene.kitti_like_sequence(4, 1242, 375, n_objects=3, seed=1003, device="cpu", start=60)
    frames = scene.to_numpy_frames(seq)
    ctx.reset()
    tr = oracle_mod.Tracker(1242, 375, K_KITTI, 387.5744, 0, 2000)
    nmax, nan_seen = 0, False
    for i, f in enumerate(frames):
        s = split_labels(f["sem"])
        o = tr.track(f["bgr"], f["disp"], f["flow"], s)
        g = ctx.track(f["bgr"], f["disp"], f["flow"], s)
        p, c, bad = compare.compare_frame(g, o)[:3]
        assert not bad and p < POSE_TOL and c < CENTRE_TOL, (i, p, c, bad)
        nmax = max(nmax, len(g["objects"]))
        nan_seen = nan_seen or any(ob["n_solve"] == 0 and np.isnan(ob["centre_pre"]).all()
                                   for ob in g["objects"])
    assert nmax == 10
    assert nan_seen  # the frame-1 object whose RANSAC keeps no inliers


def test_track_c3_long_sequence_matches_oracle(oracle_mod):
    """640 frames of the bench's own C3 sequence (seed 1003) through the bench's entry point
    (mmt_track_rgbd_chunk_device, 128-frame chunks, deferred object results as the bench runs
    them) against the oracle frame by frame: the chained map tracking (keyframes, local map,
    motion model, the synchronous LocalMapping with its local BA), flow solves and object solves
    stay within the bar over the whole chain, map tracking holds on every frame (round 4's build
    lost it near frame 337 and never recovered), and the LocalMapping counters match."""
    import torch
    import multimot_track_amd as M
    from multimot_track_amd import scene
    from oracle import compare
    n, C = 640, 128
    dev = torch.device("cuda:0")
    seq = scene.kitti_like_sequence(n, 1242, 375, n_objects=3, seed=1003, device=dev)
    ctx = M.Context(M.kitti03_config(1242, 375, 2000, max_batch=C))
    ctx.set_deferred_objects(True)
    raws = []
    try:
        for s0 in range(0, n, C):
            sl = slice(s0, min(n, s0 + C))
            raws.append(ctx.track_chunk_device(seq["bgr"][sl], seq["disp"][sl], seq["flow"][sl],
                                               seq["mask"][sl], parse=False))
        flushed = ctx.flush_objects()
        mc = ctx.map_counters()
    finally:
        ctx.close()
    import bench
    got = bench.assemble(raws, C, flushed)
    tr = oracle_mod.Tracker(1242, 375, K_KITTI, 387.5744, 0, 2000)
    ora = []
    for i in range(n):
        f = scene.to_numpy_frames({k: seq[k][i:i + 1] for k in ("bgr", "disp", "flow", "mask")})[0]
        ora.append(tr.track(f["bgr"], f["disp"], f["flow"], f["sem"]))
    rec = compare.parity_record(got, ora)
    print(rec)
    assert rec["first_divergent_frame"] is None, rec
    assert rec["lm_stop_flips"] <= compare.lm_flip_budget(n), rec
    assert [i for i, g in enumerate(got) if g["map_state"] != 1] == []
    assert sum(g["new_keyframe"] for g in got) > 60
    assert min(len(g["objects"]) for g in got[1:]) >= 1
    om = tr.map_stats()
    for k in ("n_ba", "n_fused", "n_culled", "n_ba_erased"):
        assert int(mc[k]) == om[k], (k, mc[k], om[k])
    assert om["n_ba"] > 60
    # ego relative pose error per frame step against the renderer's ground truth (the bench's
    # parity record carries the same numbers): the GPU's equals the oracle's, and both stay inside
    # the bounds the drift ablation measured for this sequence (median
    # 0.8 mm; p95 27-30 mm from the steps after a local BA moves the reference keyframe)
    rg, ro = bench.ego_rpe(got, seq["Tcw"]), bench.ego_rpe(ora, seq["Tcw"])
    print("ego RPE gpu", rg, "oracle", ro)
    for k in ("trans_m_median", "trans_m_p95", "rot_deg_median", "rot_deg_p95"):
        assert abs(rg[k] - ro[k]) < 1e-4 + 1e-3 * abs(ro[k]), (k, rg, ro)
    assert rg["trans_m_median"] < 2e-3 and rg["trans_m_p95"] < 0.06, rg
    assert rg["rot_deg_median"] < 0.02 and rg["rot_deg_p95"] < 0.2, rg


def test_lost_frame_and_relocalization_match_oracle(oracle_mod):
    """A textureless frame (no ORB keys) loses map tracking and the relocalization substitute
    recovers on the next frame (the reference keyframe's and its covisibles' map points at the
    motion model's prediction, Tracking.cc:3700-3770's acceptance): the GPU tracker takes the
    same LOST -> OK path as the oracle, frame by frame within the bar."""
    import torch
    import multimot_track_amd as M
    from multimot_track_amd import scene
    from oracle import compare
    n, C = 56, 16
    dev = torch.device("cuda:0")
    seq = scene.kitti_like_sequence(n, 1242, 375, n_objects=3, seed=1003, device=dev)
    seq["bgr"][40] = 128
    ctx = M.Context(M.kitti03_config(1242, 375, 2000, max_batch=C))
    got = []
    try:
        for s0 in range(0, n, C):
            sl = slice(s0, min(n, s0 + C))
            got += ctx.track_chunk_device(seq["bgr"][sl], seq["disp"][sl], seq["flow"][sl],
                                          seq["mask"][sl])
    finally:
        ctx.close()
    tr = oracle_mod.Tracker(1242, 375, K_KITTI, 387.5744, 0, 2000)
    ora = []
    for i in range(n):
        f = scene.to_numpy_frames({k: seq[k][i:i + 1] for k in ("bgr", "disp", "flow", "mask")})[0]
        ora.append(tr.track(f["bgr"], f["disp"], f["flow"], f["sem"]))
    rec = compare.parity_record(got, ora)
    assert rec["first_divergent_frame"] is None, rec
    st = [g["map_state"] for g in got]
    assert st[40] == 2 and all(v == 1 for v in st[:40] + st[41:]), st


def test_split_solve_fallback_matches_oracle(oracle_mod, monkeypatch):
    """The split ego solve needs its workgroups resident together; when an exchange wait exceeds
    its bound (forced here with a one-tick bound, MMT_DEBUG_SPLIT_SPIN) the solve reports it and the
    tracker re-runs it on one workgroup: the frames still match the oracle."""
    import multimot_track_amd as M
    from multimot_track_amd import scene
    from oracle import compare
    monkeypatch.setenv("MMT_DEBUG_SPLIT_SPIN", "1")
    monkeypatch.setenv("MMT_LM_SPLIT", "4")
    seq = scene.kitti_like_sequence(24, 1242, 375, n_objects=0, seed=1003, device="cpu")
    frames = scene.to_numpy_frames(seq)
    ctx = M.Context(M.kitti03_config(1242, 375, 2000, max_batch=8))
    tr = oracle_mod.Tracker(1242, 375, K_KITTI, 387.5744, 0, 2000)
    try:
        for i, f in enumerate(frames):
            g = ctx.track(f["bgr"], f["disp"], f["flow"], f["sem"])
            o = tr.track(f["bgr"], f["disp"], f["flow"], f["sem"])
            p, c, bad = compare.compare_frame(g, o)[:3]
            assert not bad and p < POSE_TOL, (i, p, bad)
        assert ctx.map_counters()["d2_split_fallbacks"] > 5
    finally:
        ctx.close()


def test_error_mid_chunk_then_track_on():
    """A frame with a semantic label above 15 fails its chunk (MmtError); the frames of the
    object pipeline that the failed call left in flight are dropped, and the context tracks the
    next chunk (no job may keep pointers into the failed call's results)."""
    import torch
    import multimot_track_amd as M
    from multimot_track_amd import scene
    dev = torch.device("cuda:0")
    seq = scene.kitti_like_sequence(24, 1242, 375, n_objects=3, seed=1003, device=dev)
    ctx = M.Context(M.kitti03_config(1242, 375, 2000, max_batch=12))
    try:
        bad = seq["mask"][:12].clone()
        bad[6][bad[6] > 0] = 20
        with pytest.raises(M.MmtError):
            ctx.track_chunk_device(seq["bgr"][:12], seq["disp"][:12], seq["flow"][:12], bad)
        out = ctx.track_chunk_device(seq["bgr"][12:], seq["disp"][12:], seq["flow"][12:],
                                     seq["mask"][12:])
        assert len(out) == 12 and all(np.isfinite(o["Tcw"]).all() for o in out)
        ctx.reset()
        out = ctx.track_chunk_device(seq["bgr"][:12], seq["disp"][:12], seq["flow"][:12],
                                     seq["mask"][:12])
        assert out[-1]["map_state"] == 1
    finally:
        ctx.close()


def test_deferred_objects_match_immediate():
    """Deferred object results (mmt_set_deferred_objects): one frame per call, the object pipeline
    kept running across calls.  Every frame's ego result is the same as in immediate mode, and
    every frame's object motions arrive exactly once, in frame order, identical to the immediate
    results (the same kernels; only when the host reads them changes)."""
    import torch
    import multimot_track_amd as M
    from multimot_track_amd import scene
    n = 40
    seq = scene.kitti_like_sequence(n, 1242, 375, n_objects=3, seed=1003,
                                    device=torch.device("cuda:0"))
    A = M.Context(M.kitti03_config(1242, 375, 2000, max_batch=8))
    B = M.Context(M.kitti03_config(1242, 375, 2000, max_batch=8))
    try:
        ra = []
        for s0 in range(0, n, 8):
            ra += A.track_chunk_device(seq["bgr"][s0:s0 + 8], seq["disp"][s0:s0 + 8],
                                       seq["flow"][s0:s0 + 8], seq["mask"][s0:s0 + 8])
        B.set_deferred_objects(True)
        rb, recs = [], []
        for i in range(n):
            r = B.track_chunk_device(seq["bgr"][i:i + 1], seq["disp"][i:i + 1],
                                     seq["flow"][i:i + 1], seq["mask"][i:i + 1])[0]
            rb.append(r)
            if r["objects_frame"] >= 0:
                recs.append((r["objects_frame"], r["objects"]))
        pending = B.flush_objects()
        recs += pending
    finally:
        A.close()
        B.close()
    assert len(pending) >= 2  # the pipeline really ran behind
    assert [f for f, _ in recs] == list(range(n))
    for i in range(n):
        a, b = ra[i], rb[i]
        assert a["frame_index"] == b["frame_index"] == i and a["objects_frame"] == i
        assert np.array_equal(a["Tcw"], b["Tcw"]) and a["map_state"] == b["map_state"]
        oa, ob = a["objects"], recs[i][1]
        assert len(oa) == len(ob)
        for x, y in zip(oa, ob):
            for k in x:
                assert np.array_equal(np.asarray(x[k]), np.asarray(y[k]), equal_nan=True), (i, k)


def test_partial_flush_blocks_tracking_until_drained():
    """A flush that leaves records for a later call (res_cap below the records owed) keeps the
    order promise: tracking is refused with MMT_ESTATE until the records are drained, then goes
    on with every record delivered once, in frame order."""
    import torch
    import multimot_track_amd as M
    from multimot_track_amd import scene
    n = 12
    seq = scene.kitti_like_sequence(n, 1242, 375, n_objects=3, seed=1003,
                                    device=torch.device("cuda:0"))
    c = M.Context(M.kitti03_config(1242, 375, 2000, max_batch=8))
    sl = lambda a, b: [seq[k][a:b] for k in ("bgr", "disp", "flow", "mask")]  # noqa: E731
    try:
        c.set_deferred_objects(True)
        got = []
        for i in range(8):
            r = c.track_chunk_device(*sl(i, i + 1))[0]
            if r["objects_frame"] >= 0:
                got.append(r["objects_frame"])
        part = c.flush_objects_part(cap=1)
        assert len(part) == 1
        got += [f for f, _ in part]
        with pytest.raises(M.MmtError, match="undelivered"):
            c.track_chunk_device(*sl(8, 9))
        got += [f for f, _ in c.flush_objects()]
        for i in range(8, n):
            r = c.track_chunk_device(*sl(i, i + 1))[0]
            if r["objects_frame"] >= 0:
                got.append(r["objects_frame"])
        got += [f for f, _ in c.flush_objects()]
    finally:
        c.close()
    assert got == list(range(n))


@pytest.mark.parametrize("k", [2, 4])
def test_contexts_from_threads_match_oracle(oracle_mod, k):
    """`bench.py --seqs-per-gpu K`'s setup: K contexts on one GPU, each tracking its own sequence
    on its own stream from its own host thread (the C-ABI releases the GIL), 64 frames each in
    chunks of 16; every context matches the oracle frame by frame, so contexts share no state."""
    import torch
    from concurrent.futures import ThreadPoolExecutor
    import multimot_track_amd as M
    from multimot_track_amd import scene, shard
    from oracle import compare
    n, C, dev = 64, 16, torch.device("cuda:0")
    seqs = [scene.kitti_like_sequence(n, 1242, 375, n_objects=3, device=dev,
                                      seed=shard.sequence_seed(1003, j)) for j in range(k)]
    ctxs = [M.Context(M.kitti03_config(nfeatures=2000, max_batch=C)) for _ in range(k)]
    streams = [torch.cuda.Stream(dev) for _ in range(k)]
    torch.cuda.synchronize(dev)

    def run(j):
        s, out = seqs[j], []
        for s0 in range(0, n, C):
            sl = slice(s0, s0 + C)
            out += ctxs[j].track_chunk_device(s["bgr"][sl], s["disp"][sl], s["flow"][sl],
                                              s["mask"][sl], streams[j].cuda_stream)
        return out

    try:
        with ThreadPoolExecutor(max_workers=k) as pool:
            got = list(pool.map(run, range(k)))
    finally:
        for c in ctxs:
            c.close()
    for j in range(k):
        frames = scene.to_numpy_frames(seqs[j])
        tr = oracle_mod.Tracker(1242, 375, K_KITTI, 387.5744, 0, 2000)
        ora = [tr.track(f["bgr"], f["disp"], f["flow"], f["sem"]) for f in frames]
        rec = compare.parity_record(got[j], ora)
        assert rec["frames"] == n and rec["first_divergent_frame"] is None, (j, rec)
