"""The flow solve with its initial pose read from device memory (FlowSolveDesc::init_dev, the
path of the ego solve queued behind TrackLocalMap's PoseOptimization): on the flow cases of
lm_bits_cases (the smallest shapes of each path of k_flow_lm and k_flow_lm_split: 3 edges, the
wave and block boundaries at 64 / 65 and 256 / 257, 513 edges, the split solves with empty slices
and with three and four workgroups) the pose, the statistics and the points' centre are bit-equal to
the call that passes the pose by value.  The probe poisons the by-value copy when the device
pointer is set, so a kernel that ignored the pointer would return NaNs."""
import numpy as np
import pytest

import lm_bits_cases as C
from synth_problems import K_KITTI

pytestmark = pytest.mark.gpu
FLOW = [c["name"] for c in C.CASES if c["kind"] == "flow"]


@pytest.fixture(scope="module")
def ctx():
    import multimot_track_amd as M
    c = M.Context(M.kitti03_config(nfeatures=2000, max_batch=8))
    yield c
    c.close()


def test_cases_cover_every_path():
    n = {C.BY_NAME[k]["n"] for k in FLOW}
    assert {3, 64, 65, 256, 257, 513} <= n
    splits = {C.BY_NAME[k]["env"].get("MMT_LM_SPLIT") for k in FLOW}
    assert {"8", "3", "4"} <= splits  # 5 edges over 8 workgroups: empty slices


@pytest.mark.parametrize("name", FLOW)
def test_init_from_device_memory_keeps_the_bits(ctx, monkeypatch, name):
    case = C.BY_NAME[name]
    arrays = C.inputs(case)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    ego = case["args"] == C.EGO  # the ego solve draws its depth noise; both kinds compute the centre
    kw = dict(use_noise=ego, g0=0.37 if ego else 0.0)
    val = ctx.flow_solve_init_dev(*arrays, *case["args"], K_KITTI, False, **kw)
    dev = ctx.flow_solve_init_dev(*arrays, *case["args"], K_KITTI, True, **kw)
    assert val[0] == dev[0] == 0
    assert np.isfinite(val[1]).all() and np.isfinite(val[3]).all()
    assert np.array_equal(val[1].view(np.uint32), dev[1].view(np.uint32))
    assert val[2] == dev[2]
    assert np.array_equal(val[3].view(np.uint32), dev[3].view(np.uint32))
    if not ego:
        # without the noise the by-value call is the solve test_gpu_lm_bits.py pins
        status, pose, st = ctx.flow_solve(*arrays, *case["args"], K_KITTI)
        assert status == 0 and st == val[2]
        assert np.array_equal(pose.view(np.uint32), val[1].view(np.uint32))
