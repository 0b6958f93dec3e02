"""The local BA graphs of tests/test_gpu_ba_chain.py (all from ba_problems.ba_problem) and the
digest of their inputs.  Shared with tools/make_golden_ba_chain.py, which records the solver's
outputs for them into tests/golden/ba_chain_golden.npz."""
import hashlib

import numpy as np

from ba_problems import ba_problem

HEAVY = 2  # mmt_ba.hip's kBaHeavy: a point with more edges than this is solved by a wave

# name -> (seed, ba_problem keywords)
CASES = {
    "rejected_trial": (61, dict(n_kf=5, n_fixed=0, kf0_local=False, n_pt=300, pose_noise=0.05,
                                pix_noise=1.5, obs_per_pt=(1, 5))),
    "two_chunks": (31, dict(n_kf=72, n_fixed=64, n_pt=150, obs_per_pt=(1, 72))),
    "three_chunks": (31, dict(n_kf=140, n_fixed=134, n_pt=120, obs_per_pt=(1, 140))),
    "wg_boundary": (31, dict(n_kf=6, n_fixed=2, n_pt=257, obs_per_pt=(1, 4))),
    "no_heavy": (31, dict(n_kf=6, n_fixed=2, n_pt=64, obs_per_pt=(1, 2))),
    "no_light": (31, dict(n_kf=6, n_fixed=2, n_pt=64, obs_per_pt=(3, 4))),
}

INPUT_KEYS = ("T", "fixed", "X", "pt", "kf", "obs", "s")


def problem(name):
    seed, kw = CASES[name]
    return ba_problem(seed, **kw)[0]


def input_digest(P):
    """SHA-256 over the problem's arrays (name, dtype, shape, bytes), hex."""
    h = hashlib.sha256()
    for k in INPUT_KEYS:
        a = np.ascontiguousarray(P[k])
        h.update(("%s %s %s|" % (k, a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def edges_per_point(P):
    return np.bincount(P["pt"], minlength=len(P["X"]))


def stats_array(st):
    """local_bundle_adjustment's stats dict as five ints: iterations, trials, n_erase."""
    return np.array([st["iterations"][0], st["iterations"][1], st["trials"][0], st["trials"][1],
                     st["n_erase"]], np.int32)
