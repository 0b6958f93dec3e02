"""The host half of the object front end (csrc/mmt_objdecide.{h,cpp}: B7 decisions and B8 label
association) on the host alone: tests/objdecide_host_check.cpp runs obj_decide on the cases of
tests/objfront_cases.py (every threshold at equality and one step past it, the numbering rules, the
histogram tie, 200 seeded random cases) and its decisions must equal, exactly, those of the
restatement tests/objfront_ref_py.py and, for the edge cases, the ones worked out by hand.  Built
with g++ under UBSan and libstdc++'s assertions; no GPU, no libmmt.so."""
import os
import subprocess

import pytest

import objfront_ref_py as R
from objfront_cases import decision_cases, write_decision_cases

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "multimot_track_amd", "csrc")


@pytest.fixture(scope="module")
def host_decisions(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("objdecide")
    exe = str(tmp / "objdecide_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-D_GLIBCXX_ASSERTIONS",
           "-fsanitize=undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "objdecide_host_check.cpp"),
           os.path.join(CSRC, "mmt_objdecide.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    assert "warning" not in b.stderr, b.stderr[-4000:]
    cases = decision_cases()
    path = str(tmp / "cases.txt")
    write_decision_cases(path, cases)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "objdecide_host_check: ok" and len(lines) == len(cases) + 1
    got = []
    for ln in lines[:-1]:
        v = [int(x) for x in ln.split()]
        assert len(v) == 1 + 2 * v[0]
        got.append((v[1::2], v[2::2]))
    return cases, got


def test_host_decisions_equal_the_restatement(host_decisions):
    cases, got = host_decisions
    assert len(cases) >= 213
    kept_any = 0
    for c, g in zip(cases, got):
        exp = R.decide(c["cnt"], c["bcnt"], c["sfcnt"], c["depth_sum"], c["hist"], c["bSecond"],
                       c["last_mod"], c["last_sem"])
        assert g == (list(exp[0]), list(exp[1])), c["name"]
        kept_any += bool(g[0])
    assert kept_any > 100  # the random cases are not all empty


def test_host_decisions_equal_the_hand_worked_edges(host_decisions):
    cases, got = host_decisions
    edges = [(c, g) for c, g in zip(cases, got) if c["expect"] is not None]
    assert len(edges) == 13
    for c, g in edges:
        assert g == c["expect"], c["name"]
