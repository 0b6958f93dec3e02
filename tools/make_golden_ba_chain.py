"""Record the local BA's outputs for the graphs of tests/ba_chain_cases.py into
tests/golden/ba_chain_golden.npz: per graph T, X (float32), the erase flags, the stats
(iterations, trials, erased) and the SHA-256 of the input arrays.  Run it on the build whose
results are the yardstick (the commit BEFORE a change to the BA kernels), never on the code under
test: tests/test_gpu_ba_chain.py demands these bits.
Usage: python tools/make_golden_ba_chain.py [--out tests/golden/ba_chain_golden.npz]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ba_chain_golden.npz"))
    a = ap.parse_args()
    import multimot_track_amd as M
    import ba_chain_cases as C
    ctx = M.Context(M.kitti03_config(nfeatures=2000, max_batch=8))
    out = {}
    for name in C.CASES:
        P = C.problem(name)
        T, X, er, st = ctx.local_bundle_adjustment(P)
        T2, X2, er2, st2 = ctx.local_bundle_adjustment(P)
        assert np.array_equal(T, T2) and np.array_equal(X, X2) and np.array_equal(er, er2) \
            and st == st2, "%s: two solves differ" % name
        out[name + ".T"] = T
        out[name + ".X"] = X
        out[name + ".erase"] = er
        out[name + ".stats"] = C.stats_array(st)
        out[name + ".sha256"] = np.array(C.input_digest(P))
        print("%-15s %5d edges  iterations %s trials %s erased %d" %
              (name, len(P["pt"]), st["iterations"], st["trials"], st["n_erase"]), flush=True)
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
