// tests/objdecide_host_check.cpp -- mmt_objdecide.cpp alone on the host (test_objdecide_host.py
// builds it under UBSan and libstdc++'s assertions): reads decision cases from the file named on
// the command line and prints each case's kept semantic labels with their motion labels; the test
// compares the lines with tests/objfront_ref_py.py's decide().
//
// Input, whitespace separated: the case count; per case bSecond, the last frame's object count m,
// m nModLabel, m nSemPosition, then per label 0..15 cnt, bcnt, sfcnt and depth_sum as the float's
// bits (an unsigned integer), then the 16 x 16 histogram.  Output per case: the kept count, then
// label and LabId pairs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../multimot_track_amd/csrc/mmt_objdecide.h"

static long long next(FILE* f) {
  long long v;
  if (std::fscanf(f, "%lld", &v) != 1) {
    std::printf("FAILED: short input\n");
    std::exit(1);
  }
  return v;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  const int ncases = (int)next(f);
  for (int c = 0; c < ncases; c++) {
    const bool bSecond = next(f) != 0;
    const int m = (int)next(f);
    std::vector<int> mod(m), sem(m);
    for (int& v : mod) v = (int)next(f);
    for (int& v : sem) v = (int)next(f);
    std::vector<mmt::LabelStats> stats(mmt::kMaxLabel);
    for (mmt::LabelStats& s : stats) {
      std::memset(&s, 0, sizeof(s));
      s.cnt = (int)next(f);
      s.bcnt = (int)next(f);
      s.sfcnt = (int)next(f);
      s.members = s.cnt;
      const uint32_t bits = (uint32_t)next(f);
      std::memcpy(&s.depth_sum, &bits, 4);
    }
    std::vector<int> hist(mmt::kMaxLabel * mmt::kMaxLabel);
    for (int& v : hist) v = (int)next(f);
    const mmt::ObjDecision d = mmt::obj_decide(stats.data(), hist.data(), bSecond, mod, sem);
    if (d.labels.size() != d.LabId.size()) {
      std::printf("FAILED: case %d: %zu labels, %zu ids\n", c, d.labels.size(), d.LabId.size());
      return 1;
    }
    std::printf("%zu", d.labels.size());
    for (size_t i = 0; i < d.labels.size(); i++) std::printf(" %d %d", d.labels[i], d.LabId[i]);
    std::printf("\n");
  }
  std::fclose(f);
  std::printf("objdecide_host_check: ok\n");
  return 0;
}
