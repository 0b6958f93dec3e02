"""The CPU oracle's object front end (oracle/track_ref.cpp: B1, B2, B4, B6-B8) against the
independent restatement tests/objfront_ref_py.py on the kitti_sample frames (real data).  The
oracle was written beside the kernels; the restatement was written from the reference alone, so a
reading the oracle and the kernels share shows here.  CPU only."""
import numpy as np
import pytest

import objfront_ref_py as R
from synth_problems import K_KITTI

BF = 387.5744
W, H = 1242, 375


def restated_frame(f, keys_xy):
    """A2, B1, B2 of one fixture frame."""
    gray, depth = R.gray_depth(f["bgr"], f["disp"], BF)
    return dict(gray=gray, depth=depth,
                b1=R.object_samples_vec(depth, f["flow"], f["sem"]),
                b2=R.static_samples(keys_xy, depth, f["flow"], f["sem"]))


def restated_objects(cur, prev, f, Tcur, Tlast):
    """B4, B6, B7, B8 of one frame after the first: (hand-off, groups, kept labels, LabId)."""
    ho = R.handoff_vec(prev["b2"]["corres"], prev["b1"]["corres"], cur["depth"], f["sem"])
    g = R.groups(ho["okeys"], ho["odepth"], ho["olabel"], prev["b1"]["keys"], prev["b1"]["depth"],
                 prev["b1"]["label"], Tcur, Tlast, K_KITTI, W, H)
    kept, lab_id = R.decide(g["cnt"], g["bcnt"], g["sfcnt"], g["depth_sum"], g["hist"], False,
                            prev["nMod"], prev["nSem"])
    return ho, g, kept, lab_id


@pytest.fixture(scope="module")
def oracle_run(oracle_mod, kitti_frames):
    tr = oracle_mod.Tracker(W, H, K_KITTI, BF, 0, 2000)
    out = []
    for f in kitti_frames:
        r = tr.track(f["bgr"], f["disp"], f["flow"], f["sem"])
        out.append(dict(n_static=r["n_static"], n_obj_samples=r["n_obj_samples"],
                        Tcw=r["Tcw"].copy(), n_keys=r["n_keys"],
                        objects=[(o["sem_label"], o["label"], o["n_points"]) for o in r["objects"]]))
    return out


def test_restated_front_end_gives_the_oracle_trackers_frames(oracle_mod, kitti_frames, oracle_run):
    prev = None
    n_objects = 0
    for t, (f, o) in enumerate(zip(kitti_frames, oracle_run)):
        gray = R.gray_depth(f["bgr"], f["disp"], BF)[0]
        assert np.array_equal(gray, oracle_mod.gray_from_bgr(f["bgr"]))
        kps, _ = oracle_mod.orb_extract(gray, 2000)
        assert len(kps) == o["n_keys"]
        cur = restated_frame(f, np.stack([kps["x"], kps["y"]], 1))
        if prev is None:
            # the first frame's samples are its own (Tracking.cc:579-586)
            assert o["n_static"] == cur["b2"]["count"] > 500
            assert o["n_obj_samples"] == cur["b1"]["count"] > 500
            cur["nMod"], cur["nSem"] = [], []
        else:
            ho, g, kept, lab_id = restated_objects(cur, prev, f, o["Tcw"], prev["Tcw"])
            assert o["n_static"] == ho["ns"] == prev["b2"]["count"], t
            assert o["n_obj_samples"] == ho["no"] == prev["b1"]["count"], t
            # exact: both sides follow the same float32 formula.  (The issue's tie rule, leaving
            # out a label whose decision hangs on samples within 1e-3 of the 0.12 threshold, is
            # not needed on these frames.)
            got = [(l, i, int(g["cnt"][l])) for l, i in zip(kept, lab_id)]
            assert got == o["objects"], (t, got, o["objects"])
            n_objects += len(got)
            cur["nMod"], cur["nSem"] = lab_id, kept
        cur["Tcw"] = o["Tcw"]
        prev = cur
    assert n_objects >= 4  # the fixture has moving cars in every frame pair
