"""Time the stereo Frame constructor against the extraction it contains ("Stereo
frames").  Workload: kitti_sample frame 0 (1242 x 375, 2,000 features per side) and a right image
made of four row bands at disparities 3, 20, 60 and 110 (tests/stereo_cases.py).

  (a) mmt_orb_extract_batch of the pair         existing code, the yardstick
  (b) mmt_stereo_frame of the pair              the same extraction + row table, matcher, median
  (c) b - a                                     the matching stage

Both calls start from host images and end synchronised with their results on the host.  (a) and
(b) alternate inside one loop after a warm-up; each is timed with a pair of HIP events (recorded on
an idle device, so they bracket the call) and with the host clock; the medians of --runs runs and
the quartiles are printed as one JSON line.  Under `rocprofv3 --kernel-trace --stats -- python
tools/stereo_bench.py` the per-kernel times (k_stereo_*).

Usage: python tools/stereo_bench.py [--runs 30] [--warmup 5]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multimot_track_amd as M  # noqa: E402
import stereo_cases as C  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert a.runs >= 20
    left, right, nf = C.pair("kitti_banded")
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    h, w = left.shape
    ctx = M.Context(M.kitti03_config(w, h, nf, max_batch=2))
    L, p = M.lib(), M._p
    cap = ctx.capacity()
    kps = np.zeros((2, cap), M.KP_DTYPE)
    desc = np.zeros((2, cap, 32), np.uint8)
    ns = np.zeros(2, np.int32)
    uR, depth = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    ridx, sem = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    ptrs = (ctypes.c_void_p * 2)(left.ctypes.data, right.ctypes.data)
    cnt = M.MmtStereoCounters()

    def extract():
        ctx._check(L.mmt_orb_extract_batch(ctx.handle, ptrs, 2, w, p(kps), p(desc), cap, p(ns)))

    def frame():
        ctx._check(L.mmt_stereo_frame(ctx.handle, p(left), p(right), w, h, w, None, p(kps[0]),
                                      p(desc[0]), cap, p(ns[0:1]), p(kps[1]), p(desc[1]), cap,
                                      p(ns[1:2]), p(uR), p(depth), p(ridx), p(sem),
                                      ctypes.byref(cnt)))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    for _ in range(a.warmup):
        extract()
        frame()
    ev = {"extract": [], "frame": []}
    host = {"extract": [], "frame": []}
    for _ in range(a.runs):
        for name, fn in (("extract", extract), ("frame", frame)):
            e, t = timed(fn)
            ev[name].append(e)
            host[name].append(t)
    q = lambda v: [round(float(x), 4) for x in np.percentile(v, (25, 50, 75))]  # noqa: E731
    out = dict(workload="%dx%d nfeatures=%d banded pair" % (w, h, nf), runs=a.runs,
               n_left=int(ns[0]), n_right=int(ns[1]), survivors=int((uR[:ns[0]] >= 0).sum()),
               counters={k: int(v) if k != "th_dist" else float(v)
                         for k, v in cnt.as_dict().items()},
               extract_ms_q25_50_75=q(ev["extract"]), frame_ms_q25_50_75=q(ev["frame"]),
               extract_host_ms_q25_50_75=q(host["extract"]), frame_host_ms_q25_50_75=q(host["frame"]),
               matching_ms=round(float(np.median(ev["frame"]) - np.median(ev["extract"])), 4),
               matching_host_ms=round(float(np.median(host["frame"]) -
                                            np.median(host["extract"])), 4))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
