"""bench.py --dump-outputs: the arrays written for one step's per-frame results (CPU), and on the
GPU what a plain run and a --full run put on the line (bench.main in this process, 8-frame
chunks)."""
import json
import os

import numpy as np
import pytest

import bench

LEGS = ("cpu_baseline", "parity", "rank_parity")


def _bench_line(argv, capsys):
    import torch
    try:
        assert bench.main(["--gpus", "1", "--chunk", "8"] + argv) == 0
    finally:  # main makes a stream of its own current
        torch.cuda.set_stream(torch.cuda.default_stream())
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_its_steps_only_and_dumps_the_last_one(tmp_path, capsys):
    out = tmp_path / "dump"
    d = _bench_line(["--steps", "3", "--warmup", "1", "--dump-outputs", str(out)], capsys)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["frames_timed"] == 3 * 8
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["ms_per_step"] == pytest.approx(8 / d["value"] * 1e3, rel=1e-3)
    assert all(d[k] is None for k in LEGS)
    assert d["config"]["c2"] is None and d["config"]["one_frame_per_call"] is None
    tcw = np.load(str(out / "Tcw.npy"))
    st = np.load(str(out / "frame_stats.npy"))
    assert tcw.dtype == np.float32 and tcw.shape == (8, 4, 4) and np.isfinite(tcw).all()
    # the last of 1 + 3 chunks: frames 24-31
    assert st[:, bench.FRAME_STATS.index("frame_index")].tolist() == list(range(24, 32))
    assert np.load(str(out / "object_motion.npy")).shape[:2] == (8, 15)


@pytest.mark.gpu
def test_full_run_adds_the_legs(capsys):
    d = _bench_line(["--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "0.2",
                     "--cpu-seqs", "0", "--c2-steps", "1", "--single-frames", "8"], capsys)
    assert d["frames_timed"] == 16
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["c2_value"] > 0
    assert d["parity"]["frames"] > 8 and d["parity"]["first_divergent_frame"] is None
    assert d["config"]["c2"]["frames"] == 8 and d["config"]["one_frame_per_call"]["frames"] == 8


def _frame(i, nobj):
    rng = np.random.default_rng(i)
    objs = [dict(label=j + 1, sem_label=j + 1, n_points=100 + j, n_inliers=90, ransac_inliers=95,
                 mm_inliers=80, n_solve=2, iterations=5,
                 init=rng.random((4, 4)).astype(np.float32),
                 X=rng.random((4, 4)).astype(np.float32),
                 motion=rng.random((4, 4)).astype(np.float32),
                 centre_pre=rng.random(3).astype(np.float32)) for j in range(nobj)]
    return dict(initialized=True, Tcw=rng.random((4, 4)).astype(np.float32), n_keys=2000 + i,
                n_obj_samples=300, ego_iterations=4, ego_inliers=1500, objects=objs, map_state=1,
                map_matches_mm=400, map_inliers_local=350, n_keyframes=7, n_mappoints=3000,
                new_keyframe=i % 2, Tcw_map=rng.random((4, 4)).astype(np.float32),
                frame_index=128 + i, objects_frame=-1)


def test_dump_outputs_arrays(tmp_path):
    import multimot_track_amd as M
    frames = [_frame(i, i % 3) for i in range(5)]
    d = str(tmp_path / "out")
    bench.dump_outputs(d, frames)
    bench.dump_outputs(d, frames[:2], "rank1_seq0_")
    names = {"Tcw", "Tcw_map", "frame_stats", "object_stats", "object_motion", "object_cam_pose",
             "object_init_pose", "object_centre_pre"}
    assert set(os.listdir(d)) == {p + n + ".npy" for n in names for p in ("", "rank1_seq0_")}
    a = {n: np.load(os.path.join(d, n + ".npy")) for n in names}
    assert all(v.dtype in (np.float32, np.float64) and len(v) == 5 for v in a.values())
    assert np.array_equal(a["Tcw"][3], frames[3]["Tcw"])
    assert np.array_equal(a["Tcw_map"][4], frames[4]["Tcw_map"])
    st = dict(zip(bench.FRAME_STATS + ("n_objects",), a["frame_stats"][2]))
    assert st["frame_index"] == 130 and st["n_keys"] == 2002 and st["n_objects"] == 2
    assert a["object_motion"].shape == (5, M.MAX_OBJECTS, 4, 4)
    assert np.array_equal(a["object_motion"][2, 1], frames[2]["objects"][1]["motion"])
    assert np.array_equal(a["object_centre_pre"][1, 0], frames[1]["objects"][0]["centre_pre"])
    assert a["object_stats"][2, 1, bench.OBJECT_STATS.index("n_points")] == 101
    assert not a["object_motion"][2, 2:].any() and not a["object_stats"][0].any()
    assert len(np.load(os.path.join(d, "rank1_seq0_Tcw.npy"))) == 2
