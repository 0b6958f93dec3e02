"""The batched renderer (SequenceRenderer.frames, what sequence() and so the bench and the tests
render with) against the frame-by-frame one (SequenceRenderer.frame): bit for bit the same image,
disparity, flow and labels, with every surface, all three boxes and the sky in view, across a
batch boundary and from a start frame other than 0."""
import numpy as np
import pytest
import torch

from multimot_track_amd import scene


def _check(dev, W, H, scale, n, start, batch, objects):
    K = {k: v * scale for k, v in scene.KITTI03.items()}
    R = scene.SequenceRenderer(scene.StreetScene(objects, 1003), W, H, K=K, device=dev)
    seq = R.sequence(n, start=start, batch=batch)
    labels, surfaces = set(), 0
    for i in range(n):
        ref = R.frame(start + i)
        for name, want in zip(("bgr", "disp", "flow", "mask"), ref):
            got = seq[name][i]
            assert got.dtype == want.dtype and got.shape == want.shape
            if got.dtype == torch.float32:  # the bits, not the values (-0.0, NaN)
                got, want = got.view(torch.int32), want.view(torch.int32)
            assert torch.equal(got, want), (name, start + i)
        labels |= set(np.unique(seq["mask"][i].cpu().numpy()).tolist())
        surfaces = max(surfaces, len(np.unique(seq["disp"][i].cpu().numpy())))
    assert labels == set(range(objects + 1)) and surfaces > 100  # the boxes are in view
    T = np.stack([np.linalg.inv(R.scene.Twc(start + i)) for i in range(n)])
    assert np.array_equal(seq["Tcw"], T)


def test_batched_render_equals_frame_by_frame_cpu():
    _check("cpu", 310, 94, 0.25, 6, 37, 4, 3)   # batches of 4 + 2
    _check("cpu", 155, 47, 0.125, 3, 0, 1, 0)   # no boxes (C2), one frame per batch


@pytest.mark.gpu
def test_batched_render_equals_frame_by_frame_gpu():
    """At the bench's geometry on the GPU, where the sequences of the bench and of the GPU tests
    are rendered."""
    _check("cuda:0", 1242, 375, 1.0, 5, 126, 3, 3)
