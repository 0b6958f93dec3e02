"""The flow solve (D2) queued behind TrackLocalMap's PoseOptimization, its initial pose read on the
device (MMT_D2_CHAIN, mmt_tracker.hip enqueue_d2), changes nothing.

The drive is the smallest the 8-level pyramid takes (931x281, the KITTI-03 camera scaled by 0.75,
1,000 features, vocabulary loaded, 40 frames in chunks of 16, frame 24 textureless: the drive of
test_vocabulary_tracking_three_quarter_res_matches_oracle), tracked with MMT_D2_CHAIN 1 and 0.
It holds the initial frame, a lost and a relocalising frame and the lost frames after it, whose
solves the host launches, and 24 frames whose solve is queued.
"""
import contextlib
import os
import re
import sys
import tempfile

import pytest

from test_gpu_vocab import VOC, _run_gpu, _same

pytestmark = pytest.mark.gpu
W, H, NFEAT, N, CHUNK, LOST = 931, 281, 1000, 40, 16, 24
LINE = re.compile(r"flow solves \(MMT_D2_CHAIN=(\d)\) chained (\d+), host-launched (\d+), "
                  r"redone (\d+)")


@contextlib.contextmanager
def _stderr_to_file():
    """The library prints its counters to the process's stderr when the context closes."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            yield f
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)


def _run_counted(args, env):
    """One tracked drive under env: (its _run_gpu result, the profile line's four counters)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("MMT_MAP_PROFILE", "1")  # the counters, printed at destruction
        for k, v in env.items():
            mp.setenv(k, v)
        with _stderr_to_file() as f:
            run = _run_gpu(*args)
            sys.stderr.flush()
            f.seek(0)
            err = f.read().decode(errors="replace")
    m = LINE.search(err)
    assert m, err[-2000:]
    return run, tuple(int(g) for g in m.groups())


@pytest.fixture(scope="module")
def drive():
    import torch
    from multimot_track_amd import scene
    K = {k: v * 0.75 for k, v in scene.KITTI03.items()}
    R = scene.SequenceRenderer(scene.StreetScene(3, 1003), W, H, K=K,
                               device=torch.device("cuda:0"))
    seq = R.sequence(N)
    seq["bgr"][LOST] = 128
    return seq, K


def test_chained_solve_changes_nothing(drive):
    seq, K = drive
    runs = {chain: _run_counted((seq, N, CHUNK, W, H, K, K["bf"], NFEAT), {"MMT_D2_CHAIN": chain})
            for chain in ("1", "0")}
    for chain, (_, c) in runs.items():
        print("MMT_D2_CHAIN=%s: mode %d chained %d host-launched %d redone %d" % ((chain,) + c))
    for chain, (_, c) in runs.items():
        mode, chained, host, redone = c
        assert mode == int(chain)
        assert redone == 0  # the guard never fires: the queued solve read the adopted pose
        assert host > 0  # the frames without a TrackLocalMap chain: lost, relocalising
        assert (chained > 0) == (chain == "1")
        assert chained + host <= N - 1  # one solve per frame after the first, none on a reset
    base = runs["0"][0]  # the order before the change
    assert base[1]["reloc"] >= 1 and base[1]["trk_ok"] >= 1
    assert _same(runs["1"][0], base)


def _run_counters(seq, K, n):
    import multimot_track_amd as M
    cfg = M.kitti03_config(W, H, NFEAT, max_batch=CHUNK)
    cfg.fx, cfg.fy, cfg.cx, cfg.cy, cfg.bf = K["fx"], K["fy"], K["cx"], K["cy"], K["bf"]
    ctx = M.Context(cfg)
    try:
        ctx.load_vocabulary(VOC)
        got = ctx.track_chunk_device(seq["bgr"][:n], seq["disp"][:n], seq["flow"][:n],
                                     seq["mask"][:n])
        return got, ctx.map_counters()["d2_split_fallbacks"]
    finally:
        ctx.close()


def test_split_fallback_with_the_chain(drive, monkeypatch):
    """The split solve that gives up (a one-tick spin bound) is run again on one workgroup from
    the unchanged descriptor, which with the chain names the device pose: the same frames."""
    seq, K = drive
    monkeypatch.setenv("MMT_DEBUG_SPLIT_SPIN", "1")
    monkeypatch.setenv("MMT_LM_SPLIT", "4")  # (the drive's solves are below the split's threshold)
    res = {}
    for chain in ("1", "0"):
        monkeypatch.setenv("MMT_D2_CHAIN", chain)
        res[chain] = _run_counters(seq, K, 16)
        print("MMT_D2_CHAIN=%s: d2_split_fallbacks %d" % (chain, res[chain][1]))
        assert res[chain][1] > 0
    assert _same(res["1"][0], res["0"][0])
