"""The host half of loop detection (csrc/mmt_loopdetect.{h,cpp}: DetectLoopCandidates, DetectLoop,
the database's add / erase, the consistency groups) on the host alone:
tests/loop_detect_host_check.cpp computes the per-keyframe triples in plain C++ for a few hand
cases and checks the candidates and the groups.  Built with g++ under UBSan and libstdc++'s
assertions; no GPU, no libmmt.so."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "multimot_track_amd", "csrc")


def test_loop_detect_host_check(tmp_path):
    exe = str(tmp_path / "loop_detect_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-D_GLIBCXX_ASSERTIONS",
           "-fsanitize=undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "loop_detect_host_check.cpp"),
           os.path.join(CSRC, "mmt_loopdetect.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    assert "warning" not in b.stderr, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "loop_detect_host_check: ok" in r.stdout
