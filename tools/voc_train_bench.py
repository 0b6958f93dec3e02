"""Time mmt_train_vocabulary on generated clustered descriptors ("Vocabulary
training").  One warm-up run at a small size, then `--repeat` timed runs (host clock around the
call, which ends synchronised).  --numpy also times tests/voc_train_ref.py, the sequential
restatement, on the same input and checks that the two trees are the same file.  Under
`rocprofv3 --kernel-trace --stats -- python tools/voc_train_bench.py ...` the per-kernel times.

Usage: python tools/voc_train_bench.py [-n 1000000] [--images 500] [-k 10] [-L 6] [--numpy]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multimot_track_amd as M  # noqa: E402


def clustered(n, seed=1, n_centres=5000, flip=0.08):
    """n descriptors around n_centres random centres, every bit flipped with probability flip."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (n_centres, 32), dtype=np.uint8)
    out = np.empty((n, 32), np.uint8)
    for s in range(0, n, 100000):
        m = min(100000, n - s)
        out[s:s + m] = c[rng.integers(0, n_centres, m)] ^ np.packbits(rng.random((m, 256)) < flip, axis=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=1000000)
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("-L", type=int, default=6)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--numpy", action="store_true")
    a = ap.parse_args()
    imgs = [np.ascontiguousarray(x) for x in np.array_split(clustered(a.n), a.images)]
    ctx = M.Context(M.kitti03_config(1242, 375, 2000))
    ctx.train_vocabulary(imgs[:2], a.k, 2)  # warm-up: code objects loaded
    times = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        st = ctx.train_vocabulary(imgs, a.k, a.L)
        times.append(time.perf_counter() - t0)
    out = dict(n=a.n, images=a.images, k=a.k, L=a.L, gpu_s=times, stats=st)
    if a.numpy:
        import voc_train_ref as R
        t0 = time.perf_counter()
        t = R.create(imgs, a.k, a.L)
        out["numpy_s"] = time.perf_counter() - t0
        with tempfile.TemporaryDirectory() as d:
            ctx.save_vocabulary(os.path.join(d, "g.txt"))
            R.save_text(t, os.path.join(d, "r.txt"))
            out["same_file"] = open(os.path.join(d, "g.txt")).read() == open(os.path.join(d, "r.txt")).read()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
