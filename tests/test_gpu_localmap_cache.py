"""The local point list cache of TrackLocalMap (LocalPointCache, mmt_mapgraph.h): the list of
the last walk is handed out again while the keyframe list and the map's structure epoch are
unchanged, and the points' handles stay on the device while the list does.

One C3 drive with the vocabulary (KITTI-03 camera, seed 1003, 160 frames in chunks of 32, frame 90
textureless: keyframes, fusions, culled points, the local BA's erasures and a relocalisation, every
kind of edit the epoch has to see), tracked with MMT_LOCALMAP_CACHE at 2 (verify: every hit is
walked again and compared, a difference throws), 1 (the default) and 0 (a walk every time, the
behaviour before the cache): per-frame outputs, vocabulary counters and the final map equal.
"""
import re

import pytest

from test_gpu_vocab import _run_gpu, _same

pytestmark = pytest.mark.gpu


def test_local_point_list_cache_changes_nothing(monkeypatch, capfd):
    import torch
    from multimot_track_amd import scene
    K = dict(scene.KITTI03)
    R = scene.SequenceRenderer(scene.StreetScene(3, 1003), 1242, 375, K=K,
                               device=torch.device("cuda:0"))
    n = 160
    seq = R.sequence(n)
    seq["bgr"][90] = 128
    args = (seq, n, 32, 1242, 375, K, 387.5744, 2000)
    monkeypatch.setenv("MMT_MAP_PROFILE", "1")  # the cache and speculation counters, at destruction
    runs, counts = {}, {}
    for mode in ("2", "1", "0"):
        monkeypatch.setenv("MMT_LOCALMAP_CACHE", mode)
        capfd.readouterr()
        runs[mode] = _run_gpu(*args)  # verify mode: a cached list that differs from the walk raises
        err = capfd.readouterr().err
        m = re.search(r"speculated (\d+) times, taken (\d+); local point list cache "
                      r"\(MMT_LOCALMAP_CACHE=(\d)\) hits (\d+), rebuilds (\d+)", err)
        assert m, err[-2000:]
        counts[mode] = tuple(int(g) for g in m.groups())
        print("MMT_LOCALMAP_CACHE=%s: speculated %d taken %d mode %d hits %d rebuilds %d"
              % ((mode,) + counts[mode]))
    for mode in ("2", "1", "0"):
        tries, taken, got_mode, hits, rebuilds = counts[mode]
        assert got_mode == int(mode)
        assert tries > taken > 0  # the speculation both taken and discarded
        assert rebuilds > 0
    # both paths ran with the cache on; without it every call walks
    assert counts["2"][3] > 0 and counts["1"][3] > 0 and counts["0"][3] == 0
    assert counts["2"][3:] == counts["1"][3:]
    # the same calls in all three runs: a call is a hit or a rebuild
    assert sum(counts["1"][3:]) == sum(counts["0"][3:])
    assert runs["1"][1]["reloc"] >= 1 and runs["1"][1]["kfdb"] > 5
    assert _same(runs["2"], runs["1"])
    assert _same(runs["1"], runs["0"])
