"""Record the outputs of the cases of tests/pnp_bits_cases.py into tests/golden/pnp_golden.npz: per
D5 case R and t (float64), the sorted inlier list, iterations and best_iter; per D6 case the
returned pose and mask, the state's best pose and mask and every integer; per stage-B run and frame
each object's label, n_points, ransac_inliers, mm_inliers, n_solve, init and X; and the SHA-256 of
every case's inputs.  Run it on the build whose results are the yardstick (the commit BEFORE a
change to csrc/mmt_pnp.hip or k_obj_stage_b; select its library with MMT_LIB_PATH), never on the
code under test: tests/test_gpu_pnp_bits.py demands these bits.  Every case is solved twice; an
output that differs between the two solves is reported and left out, the case's other outputs stay.
Usage: python tools/make_golden_pnp.py [--out tests/golden/pnp_golden.npz]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pnp_golden.npz"))
    a = ap.parse_args()
    import multimot_track_amd as M
    import pnp_bits_cases as C
    from oracle import oracle as O
    O.build()
    print("library: %s" % os.environ.get("MMT_LIB_PATH", M.LIB_PATH), flush=True)
    ctx = M.Context(M.kitti03_config(nfeatures=2000, max_batch=8))
    out, left_out = {}, []
    for case in C.CASES:
        arrays = C.inputs(case)
        draws = C.randi(O, case) if case["kind"] == "d6" else None
        r = C.solve(ctx, case, arrays, draws)[1]
        again = C.solve(ctx, case, arrays, draws)[1]
        assert r.keys() == again.keys()
        differ = [k for k in r if not np.array_equal(r[k], again[k], equal_nan=True)]
        print("%-14s %s%s" % (case["name"], r["stats"].tolist() if "stats" in r else
                              [v.shape[0] for k, v in r.items() if k.endswith(".ints")],
                              "  NOT REPEATABLE, left out: %s" % differ if differ else ""),
              flush=True)
        left_out += ["%s.%s" % (case["name"], k) for k in differ]
        for k, v in r.items():
            if k not in differ:
                out["%s.%s" % (case["name"], k)] = v
        out[case["name"] + ".sha256"] = np.array(C.input_digest(case, arrays, draws))
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes); left out: %s" % (a.out, os.path.getsize(a.out), left_out or "none"))


if __name__ == "__main__":
    main()
