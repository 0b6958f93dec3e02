// tests/loop_detect_host_check.cpp -- mmt_loopdetect.cpp alone on the host (test_loop_detect_host.py
// builds it under UBSan and libstdc++'s assertions): the triples k_loop_score would write are
// computed here by a plain merge of the two vectors, and the candidates and the consistency groups
// of a few hand cases (the ones of tests/loop_detect_cases.py, L1 scoring, values exact binary
// fractions) are checked against values worked out by hand.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../multimot_track_amd/csrc/mmt_loopdetect.h"

using mmt::LoopDetector;
using mmt::LoopScore;
using mmt::LoopSlotTable;
typedef std::vector<int32_t> Ids;

#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);          \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

struct Vec {
  std::vector<uint32_t> w;
  std::vector<double> v;
};

struct Graph {
  int n;
  std::vector<Ids> ordered, conn;
  std::vector<uint8_t> bad;
  std::vector<int32_t> os, ol, cs, cl;
  explicit Graph(int n_) : n(n_), ordered(n_), conn(n_), bad(n_, 0) {}
  mmt_covis_graph c() {
    auto csr = [&](const std::vector<Ids>& rows, std::vector<int32_t>& s, std::vector<int32_t>& l) {
      s.assign(1, 0);
      l.clear();
      for (const Ids& r : rows) {
        l.insert(l.end(), r.begin(), r.end());
        s.push_back((int32_t)l.size());
      }
      l.push_back(0);  // never read
    };
    csr(ordered, os, ol);
    csr(conn, cs, cl);
    mmt_covis_graph g;
    g.n_kf = n;
    g.ordered_start = os.data();
    g.ordered = ol.data();
    g.conn_start = cs.data();
    g.conn = cl.data();
    g.bad = bad.data();
    return g;
  }
};

struct World {
  LoopSlotTable T;
  LoopDetector D;
  std::map<int, Vec> vec;
  World() { D.reset(0); }
  void set(int id, std::vector<uint32_t> w, std::vector<double> v) {
    CHECK(T.find(id) < 0 && w.size() == v.size());
    mmt::LoopSlot s;
    s.kf_id = id;
    s.len = (int32_t)w.size();
    T.index[id] = (int32_t)T.slots.size();
    T.slots.push_back(s);
    vec[id] = Vec{w, v};
  }
  // the kernel's record, by Vocabulary::score's loop over the common words (L1)
  std::vector<LoopScore> scores(int q) {
    std::vector<LoopScore> out;
    const Vec& a = vec[q];
    for (const mmt::LoopSlot& s : T.slots) {
      const Vec& b = vec[s.kf_id];
      LoopScore r{0, INT_MAX, 0.0};
      size_t i = 0, j = 0;
      while (i < a.w.size() && j < b.w.size()) {
        if (a.w[i] == b.w[j]) {
          r.sum += std::fabs(a.v[i] - b.v[j]) - std::fabs(a.v[i]) - std::fabs(b.v[j]);
          if (r.common++ == 0) r.first = (int32_t)i;
          i++, j++;
        } else if (a.w[i] < b.w[j]) {
          i++;
        } else {
          j++;
        }
      }
      out.push_back(r);
    }
    return out;
  }
  Ids cand(int q, float min_score, Graph& g) {
    Ids out;
    const std::vector<LoopScore> sc = scores(q);
    const mmt_covis_graph cg = g.c();
    CHECK(D.candidates(T, sc.data(), q, min_score, cg, out));
    return out;
  }
  mmt_loop_result detect(int q, int last, Graph& g, Ids& cand, Ids& enough, bool ok = true) {
    mmt_loop_result r;
    const std::vector<LoopScore> sc = scores(q);
    const mmt_covis_graph cg = g.c();
    CHECK(D.detect(T, LoopDetector::early_exit(q, last) ? nullptr : sc.data(), q, last, 3, cg, 64,
                   r, cand, enough) == ok);
    return r;
  }
};

static const std::vector<uint32_t> kW8 = {1, 2, 3, 4, 5, 6, 7, 8};
static const std::vector<double> kV8(8, 0.125);

static void order_and_erase() {
  World W;
  W.set(0, {20, 21}, {0.5, 0.5});
  W.set(1, {10, 11}, {0.5, 0.5});
  W.set(2, {20, 22}, {0.5, 0.5});
  W.set(3, {10, 12}, {0.5, 0.5});
  W.set(4, {10, 20}, {0.5, 0.5});
  for (int k = 0; k < 4; k++) CHECK(W.T.db_add(k));
  CHECK(!W.T.db_add(2));   // a second add
  CHECK(!W.T.db_add(77));  // no stored vector
  Graph g(5);
  CHECK((W.cand(4, 0.f, g) == Ids{1, 3, 0, 2}));
  CHECK((W.cand(4, 0.f, g) == Ids{1, 3, 0, 2}));
  CHECK(W.T.db_erase(1));
  CHECK((W.cand(4, 0.f, g) == Ids{3, 0, 2}));
  CHECK(W.T.db_erase(1) && W.T.n_members == 3);  // erase of a non-member does nothing
  CHECK(W.T.db_add(1));
  CHECK((W.cand(4, 0.f, g) == Ids{3, 1, 0, 2}));
  Graph small(4);  // the query is outside it
  Ids out;
  const std::vector<LoopScore> sc = W.scores(4);
  CHECK(!W.D.candidates(W.T, sc.data(), 4, 0.f, small.c(), out) && !W.D.error().empty());
}

static void connected_and_min_score() {
  World W;
  W.set(0, kW8, kV8);
  W.set(1, {1, 2}, {0.5, 0.5});
  W.set(2, kW8, kV8);
  W.T.db_add(0);
  W.T.db_add(1);
  Graph g(3);
  g.conn[2] = {0};
  CHECK((W.cand(2, 0.25f, g) == Ids{1}));                       // si == minScore passes
  CHECK(W.cand(2, std::nextafterf(0.25f, 1.f), g).empty());
  Graph free(3);
  CHECK((W.cand(2, 0.25f, free) == Ids{0}));  // 8 common words now count: minCommonWords 6
}

static void common_words_cut_duplicate() {
  {
    World W;
    W.set(0, {1, 2, 3, 4, 5}, {0.25, 0.25, 0.25, 0.125, 0.125});
    W.set(1, {1, 2, 3, 4}, {0.25, 0.25, 0.25, 0.25});
    W.set(2, {4, 5, 6, 7, 8}, {0.125, 0.125, 0.25, 0.25, 0.25});
    W.set(3, kW8, kV8);
    for (int k = 0; k < 3; k++) W.T.db_add(k);
    const std::vector<LoopScore> sc = W.scores(3);
    CHECK(sc[0].common == 5 && sc[1].common == 4 && sc[2].common == 5 && sc[2].first == 3);
    CHECK(mmt::loop_finish_score(sc[1].sum, 0) == 0.5 && mmt::loop_finish_score(sc[0].sum, 0) == 0.625);
    Graph g(4);
    CHECK((W.cand(3, 0.f, g) == Ids{0, 2}));  // 4 > (int)(5 * 0.8f) = 4 fails
  }
  World W;
  W.set(0, {1, 2, 3, 4}, {0.25, 0.25, 0.25, 0.25});
  W.set(1, {1, 2, 3, 4}, {0.5, 0.25, 0.125, 0.125});
  W.set(2, {1, 2, 3, 4}, {0.5, 0.25, 0.125, 0.125});
  W.T.db_add(0);
  W.T.db_add(1);
  Graph g(3);
  CHECK((W.cand(2, 0.f, g) == Ids{1}));  // 0.75 > 0.75f * 1 fails
  g.ordered[0] = {1};
  g.ordered[1] = {0};
  CHECK((W.cand(2, 0.f, g) == Ids{1}));  // both name keyframe 1: once
}

static void detect_and_groups() {
  {
    World W;
    W.set(0, {1, 2}, {0.5, 0.5});
    W.set(1, {1, 2, 3, 4}, {0.25, 0.25, 0.25, 0.25});
    W.set(2, kW8, kV8);
    W.set(10, kW8, kV8);
    for (int k = 0; k < 3; k++) W.T.db_add(k);
    Graph g(11);
    g.ordered[10] = g.conn[10] = {0, 1};
    g.bad[0] = 1;
    Ids c, e;
    mmt_loop_result r = W.detect(10, 0, g, c, e);
    CHECK(r.ran == 1 && r.min_score == 0.5f && (c == Ids{2}) && e.empty() && r.n_groups == 1);
    CHECK(W.D.groups().size() == 1 && (W.D.groups()[0].first == Ids{2}) && W.D.groups()[0].second == 0);
    CHECK(W.T.slots[W.T.find(10)].member);
    World V;  // a non-bad covisible keyframe without a stored vector: an error, nothing changes
    V.set(10, kW8, kV8);
    Graph h(11);
    h.ordered[10] = {3};
    V.detect(10, 0, h, c, e, false);
    CHECK(!V.T.slots[0].member && V.D.groups().empty());
    h.ordered[10].clear();
    r = V.detect(10, 0, h, c, e);
    CHECK(r.ran == 1 && r.min_score == 1.f && c.empty() && V.T.slots[0].member);
  }
  World W;
  const std::vector<uint32_t> w = {1, 2, 3};
  const std::vector<double> v = {0.5, 0.25, 0.25};
  W.set(0, w, v);
  W.set(9, {50}, {1.0});
  W.set(14, {60}, {1.0});
  for (int k = 10; k < 14; k++) W.set(k, w, v);
  W.T.db_add(0);
  Graph g(15);
  g.conn[0] = {1};
  for (int k = 10; k < 14; k++)
    for (int j = 10; j < k; j++) g.conn[k].push_back(j);
  Ids c, e;
  mmt_loop_result r = W.detect(9, 0, g, c, e);
  CHECK(r.ran == 0 && c.empty() && W.T.slots[W.T.find(9)].member && W.D.groups().empty());
  for (int k = 10; k < 14; k++) {
    r = W.detect(k, 0, g, c, e);
    CHECK(r.ran == 1 && r.min_score == 1.f && (c == Ids{0}));
    CHECK(W.D.groups().size() == 1 && (W.D.groups()[0].first == Ids{0, 1}));
    CHECK(W.D.groups()[0].second == k - 10);
    CHECK(e == (k == 13 ? Ids{0} : Ids{}));
  }
  r = W.detect(14, 0, g, c, e);
  CHECK(r.ran == 1 && c.empty() && r.n_groups == 0 && W.D.groups().empty());
}

// two candidates whose groups meet one previous group, and one that meets two
static void group_loop() {
  World W;
  const std::vector<uint32_t> w = {1, 2};
  const std::vector<double> v = {0.5, 0.5};
  for (int k : {0, 1, 2, 10, 11}) W.set(k, w, v);
  for (int k = 0; k < 3; k++) W.T.db_add(k);
  Graph g(12);
  g.conn[11] = {10};
  Ids c, e;
  // keyframe 10: candidates 0, 1, 2, groups {0}, {1}, {2}, all new
  mmt_loop_result r = W.detect(10, 0, g, c, e);
  CHECK((c == Ids{0, 1, 2}) && r.n_groups == 3 && e.empty());
  // keyframe 11: candidate 0's group {0, 1} meets two previous groups, each contributes one new
  // group; candidate 1's {1} meets a group already used; candidate 2's {2} meets the third
  g.conn[0] = {1};
  r = W.detect(11, 0, g, c, e);
  CHECK((c == Ids{0, 1, 2}) && r.n_groups == 3 && e.empty());
  const auto& G = W.D.groups();
  CHECK((G[0].first == Ids{0, 1}) && G[0].second == 1);
  CHECK((G[1].first == Ids{0, 1}) && G[1].second == 1);
  CHECK((G[2].first == Ids{2}) && G[2].second == 1);
}

int main() {
  order_and_erase();
  connected_and_min_score();
  common_words_cut_duplicate();
  detect_and_groups();
  group_loop();
  std::printf("loop_detect_host_check: ok\n");
  return 0;
}
