"""Record the outputs of the single D1 / D2 / D3 solves of tests/lm_bits_cases.py into
tests/golden/lm_solves_golden.npz: per case the pose (float32 4x4), the stats (flow: status,
iterations, inliers; D1: inliers), D1's outlier flags, and the SHA-256 of the inputs.  Run it on the
build whose results are the yardstick (the commit BEFORE a change to csrc/mmt_lm.hip; select its
library with MMT_LIB_PATH), never on the code under test: tests/test_gpu_lm_bits.py demands these
bits.  Every case is solved twice; one whose two solves differ is left out and reported.
Usage: python tools/make_golden_lm_solves.py [--out tests/golden/lm_solves_golden.npz]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def solve_with_env(C, ctx, case, arrays, extra=None):
    env = dict(case["env"], **(extra or {}))
    for k, v in env.items():
        os.environ[k] = v  # the library reads its knobs per launch
    try:
        return C.solve(ctx, case, arrays)
    finally:
        for k in env:
            del os.environ[k]


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lm_solves_golden.npz"))
    a = ap.parse_args()
    import multimot_track_amd as M
    import lm_bits_cases as C
    print("library: %s" % os.environ.get("MMT_LIB_PATH", M.LIB_PATH), flush=True)
    ctx = M.Context(M.kitti03_config(nfeatures=2000, max_batch=8))
    out, left_out = {}, []
    for case in C.CASES:
        arrays = C.inputs(case)
        r = solve_with_env(C, ctx, case, arrays)
        ok = same(r, solve_with_env(C, ctx, case, arrays))
        if ok and case["chain"]:  # every trial solved for its own lambda: the same bits
            ok = same(r, solve_with_env(C, ctx, case, arrays, {"MMT_LM_MAX_CAND": "1"}))
        print("%-20s n %5d  stats %s%s" % (case["name"], case["n"], r["stats"].tolist(),
                                          "" if ok else "  NOT REPEATABLE: left out"), flush=True)
        if not ok:
            left_out.append(case["name"])
            continue
        for k, v in r.items():
            out["%s.%s" % (case["name"], k)] = v
        out[case["name"] + ".sha256"] = np.array(C.input_digest(case, arrays))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes); left out: %s" % (a.out, os.path.getsize(a.out), left_out or "none"))


if __name__ == "__main__":
    main()
