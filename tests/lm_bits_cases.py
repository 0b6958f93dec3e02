"""The single solves whose bits tests/test_gpu_lm_bits.py holds (D1 pose_optimization, D2 / D3
flow_solve, whole and split), shared with the recorder tools/make_golden_lm_solves.py: the smallest
shapes at which each path of csrc/mmt_lm.hip can go wrong.  Inputs come from synth_problems."""
import hashlib

import numpy as np

from synth_problems import K_KITTI, flow_problem, pose_opt_problem

BF = 387.5744
EGO, OBJ = (0.04, 0.3, 100), (0.01, 0.5, 200)  # rp_thres, prior information, max iterations


def _flow(name, seed, n, args, env=None, chain=False, **kw):
    return dict(kind="flow", name=name, seed=seed, n=n, args=args, env=env or {}, chain=chain, kw=kw)


def _both(tag, seed, n, **kw):
    return [_flow("%s_ego" % tag, seed, n, EGO, **kw), _flow("%s_obj" % tag, seed, n, OBJ, **kw)]


def _d1(name, seed, n, out, mono):
    return dict(kind="d1", name=name, seed=seed, n=n, env={}, chain=False,
                kw=dict(outlier_frac=out, mono_frac=mono))


_CHAIN = dict(outlier_frac=0.0, motion=0.3)  # large motion, little noise: runs of clean rejections
_CLEAN = dict(pix_noise=0.0, **_CHAIN)        # no Huber-active edge
_G2 = {"MMT_LM_SPLIT": "2"}

CASES = (
    # ---- k_flow_lm
    _both("flow3", 5, 3, outlier_frac=0.0) +                   # the minimum
    [_flow("flow37_huber", 6, 37, EGO, outlier_frac=0.3)] +     # one wave, Huber active: no closed form
    _both("flow64", 11, 64) + _both("flow65", 12, 65) +         # wave boundary of nt
    _both("flow256", 13, 256) + _both("flow257", 14, 257) +     # one item per thread / flow_lm_body<2>
    _both("flow513", 15, 513) +                                 # first item in the global item arrays
    # rejection chains on clean systems: the lambda candidate table is used
    [_flow("chain40_ego", 24, 40, EGO, chain=True, pix_noise=0.02, **_CHAIN),
     _flow("chain40_obj", 3, 40, OBJ, chain=True, pix_noise=0.0, **_CHAIN)] +
    # ---- k_flow_lm_split
    [_flow("split5_g8", 9, 5, EGO, env={"MMT_LM_SPLIT": "8"}, outlier_frac=0.0),  # empty slices
     _flow("split600_g3", 1, 600, EGO, env={"MMT_LM_SPLIT": "3"}, outlier_frac=0.1),
     _flow("split_chain900_g4", 24, 900, OBJ, env={"MMT_LM_SPLIT": "4"}, pix_noise=0.02, **_CHAIN)] +
    # flow_lm_body<2, true> (slices above 256 edges), both sides of its run-time choice, each on a
    # Huber-active system (Schur pass and its exchange, a rejected trial) and on a clean one
    # (closed-form Schur sums, candidates served after rejections).  Slices of 257: the fused
    # pass through the tile; slices of 513 (> 512): the two-pass trial, one item in the global arrays
    [_flow("split514_g2_huber", 2, 514, OBJ, env=_G2, outlier_frac=0.1),
     _flow("split514_g2_clean", 4, 514, OBJ, env=_G2, **_CLEAN),
     _flow("split1026_g2_huber", 2, 1026, OBJ, env=_G2, outlier_frac=0.1),
     _flow("split1026_g2_clean", 4, 1026, OBJ, env=_G2, **_CLEAN)] +
    # ---- D1: k_pose_opt_l<2> up to 1024 edges, <4> up to 2048, k_pose_opt beyond
    [_d1("d1_3", 8, 3, 0.0, 0.3), _d1("d1_8", 3, 8, 0.0, 0.3),  # one round (< 10 edges)
     _d1("d1_60_mono_half", 2, 60, 0.3, 0.5),
     _d1("d1_1024", 10, 1024, 0.1, 0.2), _d1("d1_1025", 11, 1025, 0.1, 0.2),
     _d1("d1_2048", 4, 2048, 0.1, 0.0), _d1("d1_2049", 6, 2049, 0.1, 0.1),
     _d1("d1_300_all_mono", 5, 300, 0.0, 1.0)])
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def inputs(case):
    """The solve's input arrays, in call order."""
    if case["kind"] == "flow":
        return flow_problem(case["seed"], case["n"], **case["kw"])[:5]  # obs, flow, depth, Tl, init
    return pose_opt_problem(case["seed"], case["n"], **case["kw"])[:4]  # Xw, obs, inv_sigma2, init


def input_digest(case, arrays):
    """SHA-256 over the case's input arrays (dtype, shape, bytes) and scalar arguments, hex."""
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s %s|" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    h.update(repr((case.get("args"), sorted(case["env"].items()), K_KITTI, BF)).encode())
    return h.hexdigest()


def solve(ctx, case, arrays):
    """The GPU solve's outputs as arrays: pose, stats, and for D1 the outlier flags."""
    if case["kind"] == "flow":
        status, pose, st = ctx.flow_solve(*arrays, *case["args"], K_KITTI)
        return dict(pose=pose, stats=np.array([status, st["iterations"], st["inliers"]], np.int32))
    n_inl, pose, outl = ctx.pose_optimization(*arrays, K_KITTI, BF)
    return dict(pose=pose, stats=np.array([n_inl], np.int32), outlier=outl)
