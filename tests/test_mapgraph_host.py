"""The map graph (csrc/mmt_mapgraph.{h,cpp}: MapPoint / KeyFrame bookkeeping, the structure epoch,
the local point list cache) on the host alone: tests/mapgraph_host_check.cpp builds a 4-keyframe,
12-point graph and checks the epoch, the cache, the bookkeeping, the local keyframe expansion and
the chunked point array against values worked out by hand from the reference's semantics.  Built
with g++ under UBSan and libstdc++'s assertions; no GPU, no libmmt.so."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "multimot_track_amd", "csrc")


def test_mapgraph_host_check(tmp_path):
    exe = str(tmp_path / "mapgraph_host_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-D_GLIBCXX_ASSERTIONS",
           "-fsanitize=undefined", "-fno-sanitize-recover=all",
           os.path.join(HERE, "mapgraph_host_check.cpp"), os.path.join(CSRC, "mmt_mapgraph.cpp"),
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    assert "warning" not in b.stderr, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "mapgraph_host_check: ok" in r.stdout
