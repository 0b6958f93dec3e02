// tests/mapgraph_host_check.cpp -- the map graph and the local point list cache on the host
// alone (csrc/mmt_mapgraph.{h,cpp}; built and run by tests/test_mapgraph_host.py under UBSan and
// libstdc++'s assertions).  Exit status 0 when every check holds.
//
// The graph: 4 keyframes of 8 keys (keys 0-4 with uR >= 0, 5-7 without; key 0 at octave 1), 12
// points.  Slots by key, every keyframe at the identity pose:
//   K0: p0 p1 p2 p3  p4 p5  p6  p7        K2: p0 p1 p2 p8 -- p10 p11 --
//   K1: p0 p1 p2 p3  p4 p5  p8  p9        K3: p0 p1 p8 p3 p9 p10 p6  --
// Shared points: K1-K0 6; K2-K0 3, K2-K1 4; K3-K0 4, K3-K1 5, K3-K2 4.  No pair reaches 15, so
// UpdateConnections links each keyframe to its single strongest neighbour, which becomes its
// parent: 0 <- 1 <- {2, 3}.  The expected values below are worked out by hand from MapPoint.cc
// and KeyFrame.cc (ties as pinned: containers keyed by KeyFrame* iterate in creation order).

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../multimot_track_amd/csrc/mmt_mapgraph.h"

using namespace mmt;
typedef std::vector<int> VI;

#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      fprintf(stderr, "line %d: CHECK(%s)\n", __LINE__, #c);   \
      exit(1);                                                 \
    }                                                          \
  } while (0)

static MapGraph g;
// ways 2, ways 1, and verify mode (every hit walked again); fresh: walks every time
static LocalPointCache c2(1, 2), c1(1, 1), cv(2, 2), fresh(0, 1);
static VI lists[2] = {{0}, {0}};  // the two alternating keyframe lists
static int turn = 0;
static VI out2, out1, outv;
static long gen2 = 0, gen1 = 0, genv = 0;

static VI walk_now(const VI& kfl) {
  VI w;
  fresh.walk(g, kfl, w);
  return w;
}

// one collect of each cache on kfl: the lists equal a fresh walk; returns whether c2's was a hit
static bool collect_all(const VI& kfl) {
  const long h = c2.hits(), r = c2.rebuilds();
  CHECK(c2.collect(g, kfl, out2, gen2));
  CHECK(c1.collect(g, kfl, out1, gen1));
  CHECK(cv.collect(g, kfl, outv, genv));  // false: a cached list differed from the walk
  const VI w = walk_now(kfl);
  CHECK(out2 == w && out1 == w && outv == w);
  CHECK(c2.hits() + c2.rebuilds() == h + r + 1);
  return c2.hits() == h + 1;
}

// after a guarded edit: the next list's first call is a rebuild, its repeat a hit of that list
static void after_bump() {
  turn ^= 1;
  const VI& kfl = lists[turn];
  const long r1 = c1.rebuilds();
  CHECK(!collect_all(kfl));
  CHECK(c1.rebuilds() == r1 + 1);
  const long gen = gen2;
  const VI was = out2;
  CHECK(collect_all(kfl));
  CHECK(gen2 == gen && out2 == was);
}
// after an edit the walk does not read: still a hit, the same generation
static void after_keep() {
  const long gen = gen2;
  CHECK(collect_all(lists[turn]));
  CHECK(gen2 == gen);
}

#define BUMPS(stmt)            \
  do {                         \
    const long e_ = g.epoch(); \
    stmt;                      \
    CHECK(g.epoch() > e_);     \
    after_bump();              \
  } while (0)
#define KEEPS(stmt)            \
  do {                         \
    const long e_ = g.epoch(); \
    stmt;                      \
    CHECK(g.epoch() == e_);    \
    after_keep();              \
  } while (0)

struct Frame {
  std::vector<mmt_kp> kps;
  std::vector<float> uR, depth;
  std::vector<uint8_t> desc;
  MapFrameH m;
  Frame(long id, uint8_t d0) : kps(8), uR(8), depth(8, 2.f), desc(8 * 32, 0) {
    for (int i = 0; i < 8; i++) {
      kps[i] = mmt_kp{10.f * i + 5.f, 5.f, 31.f, 0.f, 1.f, i == 0 ? 1 : 0, -1};
      uR[i] = i < 5 ? 10.f * i : -1.f;  // (key 0's is 0: a right coordinate, not "none")
    }
    desc[0] = d0;  // key 0's descriptor differs from keyframe to keyframe
    m.id = id;
    m.n = 8;
    m.kps = kps.data();
    m.desc = desc.data();
    m.uR = uR.data();
    m.depth = depth.data();
    m.mps.assign(8, -1);
  }
};
static const float kEye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

static int new_kf(long frame, uint8_t d0) {
  Frame f(frame, d0);
  int k = -1;
  BUMPS(k = g.new_keyframe(f.m, kEye));
  return k;
}
static int new_pt(float z, int kf) {
  const float pos[3] = {0, 0, z};
  return g.new_point_kf(pos, kf);
}
static void bind(int h, int kf, int idx) {  // AddObservation + AddMapPoint
  KEEPS(g.add_observation(h, kf, idx));
  BUMPS(g.kf_set_mp(kf, idx, h));
}
static std::vector<std::pair<int, int>> obs_of(int h) { return g.mp(h).obs(); }
static bool non_increasing(int kf) {
  const KFrame& K = g.kf(kf);
  for (size_t i = 0; i + 1 < K.ordered().size(); i++)
    if (K.conn().at(K.ordered()[i]) < K.conn().at(K.ordered()[i + 1])) return false;
  return K.ordered().size() <= K.conn().size();
}

static void check_chunk_array() {
  struct E {
    int a = 0;
    std::vector<int> v;
  };
  ChunkArray<E> arr;
  for (int i = 0; i < (1 << 13); i++) arr.push_back(E{i, {i, i + 1}});
  E& first = arr[0];
  E& last = arr[(1 << 13) - 1];
  const int* data = last.v.data();
  for (int i = 0; i < 10; i++) arr.push_back(E{-1, {}});  // crosses the 2^13 border
  CHECK(arr.size() == (size_t)(1 << 13) + 10);
  CHECK(&first == &arr[0] && &last == &arr[(1 << 13) - 1]);
  CHECK(first.a == 0 && last.a == (1 << 13) - 1 && last.v.data() == data && last.v[1] == 1 << 13);
  CHECK(arr[1 << 13].a == -1);
  // the same through the graph: a point's record across 2^13 new points
  MapGraph big;
  big.setup({1.f, 1.2f}, 2, false);
  Frame f(0, 0);
  const int k = big.new_keyframe(f.m, kEye);
  const float pos[3] = {1, 2, 3};
  const int h0 = big.new_point_kf(pos, k);
  const MPoint& p0 = big.mp(h0);
  for (int i = 0; i < (1 << 13) + 5; i++) big.new_point_kf(pos, k);
  CHECK(&p0 == &big.mp(h0) && p0.pos[2] == 3.f && big.n_points() == (size_t)(1 << 13) + 6);
  CHECK(big.n_mappoints() == (1 << 13) + 6);
}

int main() {
  check_chunk_array();
  g.setup({1.f, 1.2f}, 2, false);
  { const long e = g.epoch(); g.reset(); CHECK(g.epoch() > e); }

  // ---- K0 and its 8 points
  const int K0 = new_kf(0, 0xFF);
  CHECK(K0 == 0 && g.kf(K0).id == 0 && g.n_keyframes() == 1);
  int p[12];
  for (int i = 0; i < 8; i++) {
    p[i] = new_pt(2.f + i, K0);
    bind(p[i], K0, i);
  }
  CHECK(g.n_mappoints() == 8 && g.mp(p[0]).nObs() == 2 && g.mp(p[5]).nObs() == 1);
  KEEPS(g.add_observation(p[0], K0, 0));  // a second AddObservation of one keyframe: ignored
  CHECK(g.mp(p[0]).nObs() == 2);
  { const long e = g.epoch(); g.update_connections(K0); CHECK(g.epoch() == e); }  // no neighbour
  CHECK(g.kf(K0).parent() == -1 && g.kf(K0).ordered().empty());
  lists[0] = VI{K0};
  lists[1] = VI{K0};

  // ---- K1: p0-p5, new p8 p9
  const int K1 = new_kf(1, 0x00);
  for (int i = 0; i < 6; i++) bind(p[i], K1, i);
  p[8] = new_pt(10.f, K1);
  bind(p[8], K1, 6);
  p[9] = new_pt(11.f, K1);
  bind(p[9], K1, 7);
  BUMPS(g.update_connections(K1));
  CHECK(g.kf(K1).conn() == (std::map<int, int>{{K0, 6}}) && g.kf(K1).ordered() == VI{K0});
  CHECK(g.kf(K0).conn() == (std::map<int, int>{{K1, 6}}) && g.kf(K0).ordered() == VI{K1});
  CHECK(g.kf(K1).parent() == K0 && g.kf(K0).children() == std::set<int>{K1});
  lists[0] = VI{K0, K1};

  // ---- K2: p0 p1 p2, p8 at key 3, new p10 (key 5), p11 (key 6)
  const int K2 = new_kf(2, 0x03);
  for (int i = 0; i < 3; i++) bind(p[i], K2, i);
  bind(p[8], K2, 3);
  p[10] = new_pt(12.f, K2);
  bind(p[10], K2, 5);
  p[11] = new_pt(13.f, K2);
  bind(p[11], K2, 6);
  BUMPS(g.update_connections(K2));
  // the whole counter is kept, the ordered list holds the neighbours linked: the strongest one
  CHECK(g.kf(K2).conn() == (std::map<int, int>{{K0, 3}, {K1, 4}}) && g.kf(K2).ordered() == VI{K1});
  CHECK(g.kf(K1).conn() == (std::map<int, int>{{K0, 6}, {K2, 4}}));
  CHECK(g.kf(K1).ordered() == (VI{K0, K2}));
  CHECK(g.kf(K0).conn().count(K2) == 0);
  CHECK(g.kf(K2).parent() == K1 && g.kf(K1).children() == std::set<int>{K2});

  // ---- K3: p0 p1 p8 p3 p9 p10 p6
  const int K3 = new_kf(3, 0x07);
  const int k3pts[7] = {p[0], p[1], p[8], p[3], p[9], p[10], p[6]};
  for (int i = 0; i < 7; i++) bind(k3pts[i], K3, i);
  BUMPS(g.update_connections(K3));
  CHECK(g.kf(K3).conn() == (std::map<int, int>{{K0, 4}, {K1, 5}, {K2, 4}}));
  CHECK(g.kf(K3).ordered() == VI{K1} && g.kf(K3).parent() == K1);
  CHECK(g.kf(K1).children() == (std::set<int>{K2, K3}));
  CHECK(g.kf(K1).ordered() == (VI{K0, K3, K2}));  // weights 6, 5, 4
  lists[1] = VI{K2, K3};
  const int nobs[12] = {8, 8, 6, 6, 4, 2, 2, 1, 5, 3, 2, 1};  // 2 per key with uR >= 0, else 1
  for (int i = 0; i < 12; i++) CHECK(g.mp(p[i]).nObs() == nobs[i]);
  CHECK(obs_of(p[8]) == (std::vector<std::pair<int, int>>{{K1, 6}, {K2, 3}, {K3, 2}}));
  CHECK(g.mp(p[8]).refKF() == K1 && g.mp(p[0]).refKF() == K0 && g.mp(p[0]).firstKFid == 0);
  CHECK(g.n_mappoints() == 12 && g.n_points() == 12);
  CHECK(g.tracked_map_points(K0, 0) == 8 && g.tracked_map_points(K0, 3) == 5);
  CHECK(g.tracked_map_points(K3, 3) == 5);  // p0 p1 p8 p3 p9; p10 and p6 have 2

  // the walk itself, by hand: slot order, first visit only
  CHECK(walk_now(lists[0]) == (VI{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9]}));
  CHECK(walk_now(lists[1]) ==
        (VI{p[0], p[1], p[2], p[8], p[10], p[11], p[3], p[9], p[6]}));

  // ---- ways: alternating lists hit with 2 ways, never with 1
  {
    collect_all(lists[0]);
    collect_all(lists[1]);
    const long h2 = c2.hits(), h1 = c1.hits(), r1 = c1.rebuilds(), g0 = gen2;
    for (int i = 0; i < 6; i++) CHECK(collect_all(lists[i & 1]));
    CHECK(c2.hits() == h2 + 6 && c1.hits() == h1 && c1.rebuilds() == r1 + 6);
    CHECK(gen2 == g0);  // the list of the last call before, handed out again
    turn = 1;
  }

  // ---- edits the walk does not read
  KEEPS(g.set_pose(K2, kEye));
  KEEPS(g.compute_distinctive(p[0]));
  // key 0's descriptors 0xFF 0x00 0x03 0x07: distances to the nearest other 5 2 1 1; the median
  // of 4 is the second smallest of a row (its own 0 included); the first of the tie wins
  CHECK(g.mp(p[0]).desc[0] == 0x03 && g.mp(p[0]).desc[1] == 0 && g.mp(p[0]).desc_ver == 1);
  KEEPS(g.update_normal_depth(p[0]));
  // at (0, 0, 2), every camera at the origin; reference key at octave 1 (scale 1.2)
  CHECK(g.mp(p[0]).normal[2] == 1.f && g.mp(p[0]).normal[0] == 0.f);
  CHECK(std::fabs(g.mp(p[0]).maxDist - 2.4f) < 1e-6f && std::fabs(g.mp(p[0]).minDist - 2.f) < 1e-6f);
  KEEPS(g.erase_connection(K0, K3));  // absent
  {
    MPoint t;
    t.found = 2;
    t.visible = 3;
    int t1 = -1, t2 = -1;
    KEEPS(t1 = g.new_temp_point(t));
    KEEPS(t2 = g.new_temp_point(t));
    CHECK(t1 == MapGraph::kTemp && t2 == MapGraph::kTemp + 1);
    KEEPS(g.set_bad(t1));
    CHECK(g.mp(t1).bad() && g.n_mappoints() == 12);
    const int f0 = g.mp(p[7]).found, v0 = g.mp(p[7]).visible;
    KEEPS(g.replace(t2, p[7]));
    CHECK(g.mp(t2).bad() && g.mp(t2).replaced() == p[7] && g.n_mappoints() == 12);
    CHECK(g.mp(p[7]).found == f0 + 2 && g.mp(p[7]).visible == v0 + 3);
    KEEPS(g.clear_temps());
  }

  // ---- connections
  BUMPS(g.add_connection(K2, K3, 7));  // new
  KEEPS(g.add_connection(K2, K3, 7));  // equal weight
  BUMPS(g.add_connection(K3, K2, 6));  // 4 -> 6
  BUMPS(g.add_connection(K3, K2, 7));
  CHECK(g.kf(K2).ordered() == (VI{K3, K1, K0}) && g.kf(K3).ordered() == (VI{K2, K1, K0}));
  BUMPS(g.add_connection(K0, K3, 1));
  CHECK(g.kf(K0).ordered() == (VI{K1, K3}));
  BUMPS(g.erase_connection(K0, K3));  // present
  CHECK(g.kf(K0).ordered() == VI{K1} && g.kf(K0).conn().size() == 1);
  for (int k = 0; k < 4; k++) CHECK(non_increasing(k));

  // ---- expand_local_kfs (tree 0 <- 1 <- {2, 3}); asked: the ids the expansion tested
  {
    std::set<int> marks;
    VI asked;
    auto marked = [&](int id) { asked.push_back(id); return marks.count(id) != 0; };
    auto mark = [&](int id) { marks.insert(id); };
    // K2: its best covisible K3, no child, then its parent K1, which ends the loop: K0 is not
    // expanded (it would test K1)
    VI kfl{K2, K0};
    marks = {K2, K0};
    g.expand_local_kfs(kfl, marked, mark);
    CHECK(kfl == (VI{K2, K0, K3, K1}) && asked == (VI{K3, K1}));
    // no parent left to take: every listed keyframe is expanded
    kfl = VI{K3, K2};
    marks = {K3, K2};
    asked.clear();
    g.expand_local_kfs(kfl, marked, mark);
    CHECK(kfl == (VI{K3, K2, K1, K0}));  // K3: covisible K1; K2: covisible K0
    // more than 80 keyframes: nothing is expanded; at 80 one is, and the next is not
    kfl.assign(81, K0);
    marks = {K0};
    asked.clear();
    g.expand_local_kfs(kfl, marked, mark);
    CHECK(kfl.size() == 81 && asked.empty());
    kfl.assign(80, K0);
    g.expand_local_kfs(kfl, marked, mark);
    // K0's covisible K1 is taken, then tested again as its child; the 81st entry is not expanded
    CHECK(kfl.size() == 81 && kfl.back() == K1 && asked == (VI{K1, K1}));
  }

  // ---- Replace: p10 (K2 key 5, K3 key 5) by p11 (K2 key 6)
  g.mp(p[10]).found = 3;
  g.mp(p[10]).visible = 5;
  BUMPS(g.replace(p[10], p[11]));
  CHECK(g.mp(p[10]).bad() && g.hot(p[10]).bad() && g.mp(p[10]).replaced() == p[11]);
  CHECK(g.mp(p[10]).obs().empty() && g.n_mappoints() == 11);
  CHECK(g.kf(K2).mps()[5] == -1);     // p11 is in K2 already: the slot is erased
  CHECK(g.kf(K3).mps()[5] == p[11]);  // and not in K3: the slot is rebound
  CHECK(obs_of(p[11]) == (std::vector<std::pair<int, int>>{{K2, 6}, {K3, 5}}));
  CHECK(g.mp(p[11]).nObs() == 2 && g.mp(p[11]).found == 1 + 3 && g.mp(p[11]).visible == 1 + 5);
  KEEPS(g.replace(p[11], p[11]));  // onto itself: nothing

  // ---- EraseObservation
  KEEPS(g.erase_observation(p[8], K0));  // not an observer
  CHECK(g.mp(p[8]).nObs() == 5);
  KEEPS(g.erase_observation(p[8], K1));  // 5 -> 4: stays good, the reference moves on
  CHECK(g.mp(p[8]).nObs() == 4 && !g.mp(p[8]).bad() && g.mp(p[8]).refKF() == K2);
  CHECK(g.kf(K1).mps()[6] == p[8]);  // (the caller erases the keyframe's slot)
  BUMPS(g.kf_set_mp(K1, 6, -1));
  BUMPS(g.erase_observation(p[9], K1));  // 3 -> 2: bad, the other observer's slot emptied
  CHECK(g.mp(p[9]).bad() && g.hot(p[9]).bad() && g.mp(p[9]).refKF() == K3);
  CHECK(g.mp(p[9]).obs().empty() && g.kf(K3).mps()[4] == -1 && g.n_mappoints() == 10);
  BUMPS(g.kf_set_mp(K1, 7, -1));
  BUMPS(g.set_bad(p[7]));
  CHECK(g.mp(p[7]).bad() && g.kf(K0).mps()[7] == -1 && g.n_mappoints() == 9);

  // ---- KeyFrame::SetBadFlag of K1 (parent K0, children K2 and K3)
  { const long e = g.epoch(); g.kf_set_bad(K0); CHECK(g.epoch() == e && !g.kf(K0).bad()); }
  CHECK(g.kf(K0).ordered() == VI{K1});
  BUMPS(g.kf_set_bad(K1));
  CHECK(g.kf(K1).bad() && g.kf(K1).conn().empty() && g.kf(K1).ordered().empty());
  CHECK(g.n_keyframes() == 3 && g.n_kfs() == 4);
  CHECK(g.kf(K0).conn().empty() && g.kf(K0).ordered().empty());
  CHECK(g.kf(K2).ordered() == (VI{K3, K0}) && g.kf(K3).ordered() == (VI{K2, K0}));
  // first round: candidates {K0}; K3's link to K0 (4) beats K2's (3): K3 -> K0.  Second round:
  // candidates {K0, K3}; K2's link to K3 (7) beats its link to K0: K2 -> K3
  CHECK(g.stats().n_reparent == 2);
  CHECK(g.kf(K3).parent() == K0 && g.kf(K2).parent() == K3 && g.kf(K0).parent() == -1);
  CHECK(g.kf(K0).children() == std::set<int>{K3} && g.kf(K3).children() == std::set<int>{K2});
  for (int k = 0; k < 4; k++) {
    const KFrame& K = g.kf(k);
    if (K.bad() || K.id == 0) continue;
    CHECK(K.parent() >= 0 && !g.kf(K.parent()).bad() && g.kf(K.parent()).children().count(k));
  }
  // its observations: p0 p1 8 -> 6, p2 p3 6 -> 4, p4 4 -> 2 and p5 2 -> 1: bad
  const int nobs2[6] = {6, 6, 4, 4, 2, 1};
  for (int i = 0; i < 6; i++) CHECK(g.mp(p[i]).nObs() == nobs2[i] && g.mp(p[i]).bad() == (i >= 4));
  CHECK(g.kf(K0).mps()[4] == -1 && g.kf(K0).mps()[5] == -1 && g.n_mappoints() == 7);
  CHECK(g.mp(p[0]).refKF() == K0 && g.mp(p[0]).obs_index(K1) == -1);
  for (int k = 0; k < 4; k++) CHECK(non_increasing(k));

  // a bad keyframe in a covisibility list is skipped
  BUMPS(g.add_connection(K2, K1, 9));
  CHECK(g.kf(K2).ordered() == (VI{K1, K3, K0}));
  {
    std::set<int> marks{K2};
    VI kfl{K2};
    g.expand_local_kfs(
        kfl, [&](int id) { return marks.count(id) != 0; }, [&](int id) { marks.insert(id); });
    CHECK(kfl == (VI{K2, K3}));  // K1 skipped; K3 is its parent too
  }

  // ---- reset: an equal (empty) keyframe list is still rebuilt
  lists[0].clear();
  lists[1].clear();
  collect_all(VI{});
  BUMPS(g.reset());
  CHECK(out2.empty() && g.n_kfs() == 0 && g.n_points() == 0 && g.n_mappoints() == 0);
  CHECK(new_kf(7, 0) == 0 && g.kf(0).id == 0);  // KeyFrame::nNextId starts again
  printf("mapgraph_host_check: ok (%ld cache hits, %ld rebuilds with 2 ways; 1 way: %ld, %ld)\n",
         c2.hits(), c2.rebuilds(), c1.hits(), c1.rebuilds());
  return 0;
}
