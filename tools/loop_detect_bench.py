"""Loop detection at database sizes a long sequence reaches: N stored keyframes of 1,500 words
against a 1,500-word query of which a fraction F of each stored vector's words are the query's.
Prints, per (N, F), the wall time of one mmt_detect_loop call (C-ABI, the graph built once; the
median and the minimum over the timed calls).  Under `rocprofv3 --kernel-trace --stats` (the
program after `--`) each call is one k_loop_score dispatch, in the order printed here.
Usage: loop_detect_bench.py [--calls 20] [--warmup 3]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import multimot_track_amd as M  # noqa: E402

WORDS = 1500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = M.Context(M.kitti03_config(nfeatures=2000))
    L = M.lib()
    rng = np.random.default_rng(5)
    universe = np.arange(1000000, dtype=np.uint32)
    qwords = np.sort(rng.choice(universe[::2], WORDS, replace=False))

    def other_words(m):  # m distinct odd words
        u = np.unique(rng.integers(0, 500000, m + 200))
        return (rng.choice(u, m, replace=False) * 2 + 1).astype(np.uint32)

    nq = a.warmup + a.calls
    for n in (500, 4000):
        for frac in (0.05, 0.5):
            ctx.loop_reset(0)
            nc = int(round(WORDS * frac))
            for k in range(n):
                w = np.sort(np.concatenate([rng.choice(qwords, nc, replace=False),
                                            other_words(WORDS - nc)]))
                x = rng.uniform(0.2, 3.0, WORDS)
                ctx.loop_set_bow(k, w, x / np.abs(x).sum())
                ctx.loop_db_add(k)
            for k in range(n, n + nq):  # the queries: the same words, one id per call
                x = rng.uniform(0.2, 3.0, WORDS)
                ctx.loop_set_bow(k, qwords, x / np.abs(x).sum())
            # covisibility between temporal neighbours, the five before and after
            nk = n + nq
            rows = [[j for j in range(max(0, k - 5), min(nk, k + 6)) if j != k] for k in range(nk)]
            keep = []
            # the queries are connected to one another, so each call meets the same database
            conn = [r if k < n else sorted(set(r) | (set(range(n, nk)) - {k}))
                    for k, r in enumerate(rows)]
            g = M._covis_graph(dict(ordered=rows, conn=conn, bad=[0] * nk), keep)
            cand = np.zeros(nk, np.int32)
            enough = np.zeros(nk, np.int32)
            r = M.MmtLoopResult()
            times = []
            for i in range(nq):
                t0 = time.perf_counter()
                rc = L.mmt_detect_loop(ctx.handle, n + i, 0, 3, ctypes.byref(g), ctypes.byref(r),
                                       M._p(cand), M._p(enough), nk)
                dt = time.perf_counter() - t0
                if rc != 0:
                    raise SystemExit("mmt_detect_loop: %d" % rc)
                if i >= a.warmup:
                    times.append(dt * 1e6)
            st = ctx.loop_stats()
            print("stored %5d  common %4.0f %%  detect_loop wall median %8.1f us  min %8.1f us  "
                  "(%d calls; last: %d candidates, %d enough; min_score %.4f; word array %d "
                  "elements, grown %d times)" % (
                      n, 100 * frac, float(np.median(times)), min(times), len(times),
                      r.n_candidates, r.n_enough, r.min_score, st["word_capacity"],
                      st["word_grown"]), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
