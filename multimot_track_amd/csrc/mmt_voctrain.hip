// multimot_track_amd/csrc/mmt_voctrain.hip -- TemplatedVocabulary::create on the GPU (see
// mmt_voctrain.h).
//
// The tree is built level by level: every node of a level that runs k-means (more than k
// features) goes through the same launches.  The features are an index permutation in which a
// node's features are contiguous and keep their original relative order (the reference's
// groups[i] are filled in feature order; that order decides k-means++'s picks and the trivial
// case's child order).  A node's segment is cut into work items of at most kItem features, one
// workgroup each, so a 10^6-feature root and 10^5 ten-feature nodes fill the GPU alike.
//
//   seeding   k_seed_first, then per round k_seed_dist (Hamming distance to the node's newest
//             centre min-ed into min_dist, integer sum per item) and k_seed_pick (one wave per
//             node: dist_sum, cut_d in double from the uploaded draw, the first feature whose
//             inclusive integer prefix sum reaches it).  No host round trip per round.
//   Lloyd     k_vote (per cluster and bit the members' votes: each thread owns one of the 256
//             bits and sums it over the item's features staged in LDS grouped by cluster, so the
//             counters need no atomics; a node of one item writes its new centres
//             itself, a larger one adds its partial counts with integer global atomics),
//             k_means_multi (centres of the nodes of several items), k_assign (nearest centre,
//             strict <; per node a "changed" flag).  The host reads one flag back per iteration.
//             Converged nodes are fixed points and are skipped.
//   regroup   k_count, k_offsets, k_scatter: a stable partition of every node's segment by cluster.
//
// Every decision is an integer (distances, vote counts, prefix sums), so the result does not
// depend on the order of the atomics or the scans.

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "mmt_devbuf.h"
#include "mmt_internal.h"
#include "mmt_voctrain.h"
#include "mmt_wgscan.h"

namespace mmt {

namespace {

constexpr int kItem = 1024;  // features per work item
constexpr int kMaxK = 20;

struct VtItem {
  int node, begin, count;  // level-local node, absolute position in the permutation
};
struct VtNode {
  int start, n;        // segment in the permutation
  int item0, n_items;  // its work items
  int first;           // round 0: RandomInt(0, n - 1)
  int multi;           // index into the global vote counters (n_items > 1), or -1
};

__device__ __forceinline__ void load_desc(const uint32_t* __restrict__ desc, int f, uint32_t (&d)[8]) {
  const uint4* p = reinterpret_cast<const uint4*>(desc + 8 * (size_t)f);
  const uint4 a = p[0], b = p[1];
  d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
  d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}

// round 0 of initiateClustersKMpp: the node's first centre
__global__ __launch_bounds__(256) void k_seed_first(const VtNode* __restrict__ nodes, int nn, int k,
                                                    const uint32_t* __restrict__ desc,
                                                    const int* __restrict__ perm, uint32_t* cent,
                                                    int* ncent) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int node = t >> 3, w = t & 7;
  if (node >= nn) return;
  const VtNode nd = nodes[node];
  const int f = perm[nd.start + nd.first];
  cent[((size_t)node * k) * 8 + w] = desc[8 * (size_t)f + w];
  if (w == 0) ncent[node] = 1;
}

// min_dists against the node's newest centre and their sum over the item.  A node whose seeding
// has stopped (dist_sum 0) repeats its last centre: the minimum does not change.
__global__ __launch_bounds__(256) void k_seed_dist(const VtItem* __restrict__ items,
                                                   const uint32_t* __restrict__ desc,
                                                   const int* __restrict__ perm,
                                                   const uint32_t* __restrict__ cent,
                                                   const int* __restrict__ ncent, int k,
                                                   uint32_t* min_dist, uint32_t* item_sum) {
  __shared__ uint32_t s_part[4];
  const VtItem it = items[blockIdx.x];
  const int c = ncent[it.node] - 1;
  uint32_t ce[8];
  load_desc(cent, it.node * k + c, ce);
  uint32_t sum = 0;
  for (int i = threadIdx.x; i < it.count; i += 256) {
    const int pos = it.begin + i;
    uint32_t d[8];
    load_desc(desc, perm[pos], d);
    uint32_t h = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) h += __popc(d[j] ^ ce[j]);
    const uint32_t m = min(min_dist[pos], h);
    min_dist[pos] = m;
    sum += m;
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) item_sum[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// One wave per node, round r >= 1: dist_sum, cut_d = RandomValue(0, dist_sum) from the uploaded
// draw, and the first feature with d_up_now >= cut_d.  The sums are integers, so d_up_now >= cut_d
// is d_up_now >= ceil(cut_d).
__global__ __launch_bounds__(64) void k_seed_pick(const VtNode* __restrict__ nodes, int round, int k,
                                                  const uint32_t* __restrict__ draws,
                                                  const uint32_t* __restrict__ item_sum,
                                                  const VtItem* __restrict__ items,
                                                  const uint32_t* __restrict__ min_dist,
                                                  const uint32_t* __restrict__ desc,
                                                  const int* __restrict__ perm, uint32_t* cent,
                                                  int* ncent) {
  const int node = blockIdx.x, lane = threadIdx.x;
  if (ncent[node] != round) return;  // stopped in an earlier round
  const VtNode nd = nodes[node];
  unsigned long long total = 0;
  for (int b = 0; b < nd.n_items; b += 64) {
    uint32_t v = b + lane < nd.n_items ? item_sum[nd.item0 + b + lane] : 0u;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    total += v;
  }
  if (total == 0) return;  // dist_sum == 0: fewer than k distinct descriptors
  const double cut_d = (double)draws[(size_t)node * (k - 1) + (round - 1)] / 2147483647.0 * (double)total;
  const unsigned long long target = (unsigned long long)ceil(cut_d);
  // the item, then the feature inside it
  unsigned long long run = 0;
  int item = nd.item0 + nd.n_items - 1;
  bool found = false;
  for (int b = 0; b < nd.n_items && !found; b += 64) {
    const uint32_t v = b + lane < nd.n_items ? item_sum[nd.item0 + b + lane] : 0u;
    const uint32_t inc = wave_scan_incl(v);
    const unsigned long long hit = __ballot(run + inc >= target);
    if (hit) {
      const int l = __ffsll((long long)hit) - 1;
      item = nd.item0 + b + l;
      run += __shfl(inc, l) - __shfl(v, l);
      found = true;
    } else {
      run += __shfl(inc, 63);
    }
  }
  if (!found) {  // cannot happen (target <= total); the reference's fall-through: the last feature
    item = nd.item0 + nd.n_items - 1;
    run = total;
  }
  const VtItem it = items[item];
  int pos = nd.start + nd.n - 1;
  bool got = false;
  for (int b = 0; b < it.count && !got && found; b += 64) {
    const uint32_t v = b + lane < it.count ? min_dist[it.begin + b + lane] : 0u;
    const uint32_t inc = wave_scan_incl(v);
    const unsigned long long hit = __ballot(b + lane < it.count && run + inc >= target);
    if (hit) {
      pos = it.begin + b + __ffsll((long long)hit) - 1;
      got = true;
    } else {
      run += __shfl(inc, 63);
    }
  }
  const int f = perm[pos];
  if (lane < 8) cent[((size_t)node * k + round) * 8 + lane] = desc[8 * (size_t)f + lane];
  if (lane == 0) ncent[node] = round + 1;
}

// bit b of the new centre of a cluster of n members: FORB::meanValue's count >= n / 2 + n % 2; the
// 64 bits of a wave into two dwords
__device__ __forceinline__ void write_mean(uint32_t* dst, int wave, int lane, uint32_t cnt, int n) {
  const unsigned long long m = __ballot((int)cnt >= n / 2 + n % 2);
  if (lane == 0) {
    dst[2 * wave] = (uint32_t)m;
    dst[2 * wave + 1] = (uint32_t)(m >> 32);
  }
}

// The votes of the item's features for their clusters' new centres, from the previous
// iteration's assignment.  Thread b owns bit b: it alone updates column b of the LDS counters.
// LDS: 20 KB of counters and 9 KB of staged descriptors per workgroup.
__global__ __launch_bounds__(256) void k_vote(const VtItem* __restrict__ items,
                                              const VtNode* __restrict__ nodes,
                                              const int* __restrict__ active,
                                              const uint32_t* __restrict__ desc,
                                              const int* __restrict__ perm,
                                              const uint8_t* __restrict__ assign,
                                              const int* __restrict__ ncent, int k, uint32_t* cent,
                                              uint32_t* gcnt, uint32_t* gsize) {
  __shared__ uint32_t s_cnt[kMaxK][256];
  __shared__ uint32_t s_desc[256][9];
  __shared__ int s_n[kMaxK];       // members of each cluster among the staged features
  __shared__ int s_lo[kMaxK + 1];  // where each cluster's run starts in s_desc
  __shared__ uint32_t s_size[kMaxK];
  const VtItem it = items[blockIdx.x];
  if (!active[it.node]) return;
  const int nc = min(ncent[it.node], kMaxK), b = threadIdx.x;
  const int wd = b >> 5, sh = b & 31;
  for (int c = 0; c < nc; c++) s_cnt[c][b] = 0;
  uint32_t my_size = 0;
  // 256 features at a time are staged grouped by cluster (any order inside a cluster: the votes
  // are sums), so a thread sums its bit over a run in a register
  for (int base = 0; base < it.count; base += 256) {
    const int m = min(256, it.count - base);
    if (b < kMaxK) s_n[b] = 0;
    __syncthreads();
    uint32_t d[8];
    int a = -1, slot = 0;
    if (b < m) {
      const int pos = it.begin + base + b;
      load_desc(desc, perm[pos], d);
      a = assign[pos];
      if (a < nc) slot = atomicAdd(&s_n[a], 1);
      else a = -1;
    }
    __syncthreads();
    if (b == 0) {
      int run = 0;
      for (int c = 0; c < nc; c++) {
        s_lo[c] = run;
        run += s_n[c];
      }
      s_lo[nc] = run;
    }
    if (b < nc) my_size += (uint32_t)s_n[b];
    __syncthreads();
    if (a >= 0) {
      const int row = s_lo[a] + slot;
#pragma unroll
      for (int j = 0; j < 8; j++) s_desc[row][j] = d[j];
    }
    __syncthreads();
    for (int c = 0; c < nc; c++) {
      const int lo = s_lo[c], hi = s_lo[c + 1];
      uint32_t acc = 0;
#pragma unroll 8
      for (int f = lo; f < hi; f++) acc += (s_desc[f][wd] >> sh) & 1u;
      if (hi > lo) s_cnt[c][b] += acc;
    }
  }
  if (b < kMaxK) s_size[b] = my_size;
  __syncthreads();
  const VtNode nd = nodes[it.node];
  if (nd.multi < 0) {
    // the whole node is here.  An empty cluster keeps its centre (pinned: the reference reads a
    // released Mat); a cluster of one member keeps that member (its votes are its bits).
    for (int c = 0; c < nc; c++) {
      const int n = (int)s_size[c];
      if (n > 0) write_mean(cent + ((size_t)it.node * k + c) * 8, b >> 6, b & 63, s_cnt[c][b], n);
    }
  } else {
    for (int c = 0; c < nc; c++) {
      const uint32_t v = s_cnt[c][b];
      if (v) atomicAdd(&gcnt[((size_t)nd.multi * k + c) * 256 + b], v);
    }
    if (b < nc && s_size[b]) atomicAdd(&gsize[(size_t)nd.multi * k + b], s_size[b]);
  }
}

// New centres of the nodes of several items from the global counters, which are left zeroed.
__global__ __launch_bounds__(256) void k_means_multi(const int* __restrict__ multi_node,
                                                     const int* __restrict__ active,
                                                     const int* __restrict__ ncent, int k,
                                                     uint32_t* cent, uint32_t* gcnt, uint32_t* gsize) {
  const int mi = blockIdx.x, node = multi_node[mi], b = threadIdx.x;
  if (!active[node]) return;
  const int nc = min(ncent[node], kMaxK);
  for (int c = 0; c < nc; c++) {
    const size_t g = (size_t)mi * k + c;
    const int n = (int)gsize[g];
    const uint32_t v = gcnt[g * 256 + b];
    gcnt[g * 256 + b] = 0;
    if (n > 0) write_mean(cent + ((size_t)node * k + c) * 8, b >> 6, b & 63, v, n);
  }
  __syncthreads();
  if (b < nc) gsize[(size_t)mi * k + b] = 0;
}

// Nearest centre (strict <: the first of equal centres wins) and the node's "changed" flag.
__global__ __launch_bounds__(256) void k_assign(const VtItem* __restrict__ items,
                                                const int* __restrict__ active,
                                                const uint32_t* __restrict__ desc,
                                                const int* __restrict__ perm,
                                                const uint32_t* __restrict__ cent,
                                                const int* __restrict__ ncent, int k,
                                                uint8_t* assign, int* changed, int* any_changed) {
  __shared__ uint32_t s_cent[kMaxK][8];
  const VtItem it = items[blockIdx.x];
  if (!active[it.node]) return;
  const int nc = min(ncent[it.node], kMaxK);
  if (threadIdx.x < nc * 8)
    s_cent[threadIdx.x >> 3][threadIdx.x & 7] = cent[((size_t)it.node * k) * 8 + threadIdx.x];
  __syncthreads();
  int diff = 0;
  for (int i = threadIdx.x; i < it.count; i += 256) {
    const int pos = it.begin + i;
    uint32_t d[8];
    load_desc(desc, perm[pos], d);
    int best = 0, best_d = 257;
    for (int c = 0; c < nc; c++) {
      int h = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) h += __popc(d[j] ^ s_cent[c][j]);
      if (h < best_d) {
        best_d = h;
        best = c;
      }
    }
    if (assign[pos] != (uint8_t)best) {
      assign[pos] = (uint8_t)best;
      diff = 1;
    }
  }
  if (__syncthreads_or(diff) && threadIdx.x == 0) {
    changed[it.node] = 1;
    *any_changed = 1;
  }
}

// ---- regrouping: a stable partition of every node's segment by cluster (one wave per item)
__global__ __launch_bounds__(64) void k_count(const VtItem* __restrict__ items,
                                              const uint8_t* __restrict__ assign, int k,
                                              int* item_cnt) {
  const VtItem it = items[blockIdx.x];
  const int lane = threadIdx.x;
  int acc = 0;
  for (int b = 0; b < it.count; b += 64) {
    const bool ok = b + lane < it.count;
    const int a = ok ? assign[it.begin + b + lane] : 255;
    for (int c = 0; c < k; c++) {
      const int n = __popcll(__ballot(a == c));
      if (lane == c) acc += n;
    }
  }
  if (lane < k) item_cnt[(size_t)blockIdx.x * k + lane] = acc;
}

// per node: where each (cluster, item) run starts, and the cluster sizes
__global__ __launch_bounds__(256) void k_offsets(const VtNode* __restrict__ nodes, int nn, int k,
                                                 const int* __restrict__ item_cnt, int* item_off,
                                                 int* csize) {
  const int node = blockIdx.x * blockDim.x + threadIdx.x;
  if (node >= nn) return;
  const VtNode nd = nodes[node];
  int run = nd.start;
  for (int c = 0; c < k; c++) {
    const int run0 = run;
    for (int i = 0; i < nd.n_items; i++) {
      const size_t e = (size_t)(nd.item0 + i) * k + c;
      item_off[e] = run;
      run += item_cnt[e];
    }
    csize[(size_t)node * k + c] = run - run0;
  }
}

__global__ __launch_bounds__(64) void k_scatter(const VtItem* __restrict__ items,
                                                const VtNode* __restrict__ nodes,
                                                const uint8_t* __restrict__ assign, int k,
                                                const int* __restrict__ item_off,
                                                const int* __restrict__ perm_in, int* perm_out) {
  __shared__ int s_base[64];
  const VtItem it = items[blockIdx.x];
  const VtNode nd = nodes[it.node];
  const int lane = threadIdx.x;
  s_base[lane] = lane < k ? item_off[(size_t)blockIdx.x * k + lane] : 0;
  __syncthreads();
  for (int b = 0; b < it.count; b += 64) {
    const bool ok = b + lane < it.count;
    const int a = ok ? assign[it.begin + b + lane] : 255;
    int rank = 0, add = 0;
    for (int c = 0; c < k; c++) {
      const unsigned long long m = __ballot(a == c);
      if (a == c) rank = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == c) add = __popcll(m);
    }
    if (ok && a < k) {
      const int dst = s_base[a] + rank;
      if (dst >= nd.start && dst < nd.start + nd.n) perm_out[dst] = perm_in[it.begin + b + lane];
    }
    __syncthreads();
    s_base[lane] += add;
    __syncthreads();
  }
}

// a node waiting for its HKmeansStep: its place in the tree under construction, its segment of
// the permutation and its random key
struct Pending {
  int tnode, start, n;
  uint64_t key;
};

}  // namespace

void train_vocabulary(const uint8_t* desc, const int32_t* image_start, int n_images,
                      const mmt_voc_train_params& p, Vocabulary& out, mmt_voc_train_stats& stats,
                      hipStream_t st) {
  if (!desc || !image_start || n_images <= 0) throw ArgError("train_vocabulary: no images");
  if (p.k < 2 || p.k > kMaxK || p.L < 1 || p.L > 10)
    throw ArgError("train_vocabulary: k must be in 2..20 and L in 1..10");
  if (p.weighting < 0 || p.weighting > 3) throw ArgError("train_vocabulary: weighting must be 0..3");
  if (p.scoring < 0 || p.scoring > 1)
    throw ArgError("train_vocabulary: only the L1 / L2 norm scorings are supported");
  if (p.max_iters < 0) throw ArgError("train_vocabulary: max_iters < 0");
  if (image_start[0] != 0) throw ArgError("train_vocabulary: image_start[0] must be 0");
  for (int i = 0; i < n_images; i++)
    if (image_start[i + 1] < image_start[i])
      throw ArgError("train_vocabulary: image_start must not decrease");
  const int N = image_start[n_images];
  if (N <= 0) throw ArgError("train_vocabulary: no descriptors");
  const int k = p.k, L = p.L, max_iters = p.max_iters > 0 ? p.max_iters : 1000;
  memset(&stats, 0, sizeof(stats));

  // the tree under construction, in creation (level) order; ids are assigned afterwards.  A
  // node's children are created together: [t_first[n], t_first[n] + t_nchild[n])
  std::vector<int> t_parent{-1}, t_first{0}, t_nchild{0};
  std::vector<uint8_t> t_desc(32, 0);
  auto add_child = [&](int parent, const uint8_t* d) {
    const int id = (int)t_parent.size();
    if (t_nchild[parent]++ == 0) t_first[parent] = id;
    t_parent.push_back(parent);
    t_first.push_back(0);
    t_nchild.push_back(0);
    t_desc.insert(t_desc.end(), d, d + 32);
    return id;
  };

  DevBuf<uint32_t> d_desc(8 * (size_t)N), d_min(N);
  DevBuf<int> d_perm(N), d_perm2(N);
  DevBuf<uint8_t> d_assign(N);
  d_desc.up((const uint32_t*)desc, 8 * (size_t)N, st);
  std::vector<int> h_perm(N);
  for (int i = 0; i < N; i++) h_perm[i] = i;
  d_perm.up(h_perm, st);
  int* perm = d_perm.p;
  int* perm2 = d_perm2.p;

  std::vector<Pending> pending{{0, 0, N, voc_mix(p.seed)}}, next;
  std::vector<VtNode> nodes;
  std::vector<VtItem> items;
  std::vector<uint32_t> draws, h_cent;
  std::vector<int> multi_node, h_ncent, h_csize, h_changed;
  std::vector<uint64_t> keys;
  std::vector<int> tnode_of;
  for (int level = 1; level <= L && !pending.empty(); level++) {
    nodes.clear();
    items.clear();
    draws.clear();
    multi_node.clear();
    keys.clear();
    tnode_of.clear();
    next.clear();
    for (const Pending& q : pending) {
      if (q.n <= k) {  // trivial case: one cluster per feature, none of them recurses
        for (int i = 0; i < q.n; i++) add_child(q.tnode, desc + 32 * (size_t)h_perm[q.start + i]);
        continue;
      }
      VtNode nd;
      nd.start = q.start;
      nd.n = q.n;
      nd.item0 = (int)items.size();
      nd.n_items = (q.n + kItem - 1) / kItem;
      nd.multi = -1;
      if (nd.n_items > 1) {
        nd.multi = (int)multi_node.size();
        multi_node.push_back((int)nodes.size());
      }
      // the node's draws: RandomInt for round 0, then one RandomValue per round, a zero redrawn
      uint64_t j = 0;
      const uint32_t r0 = (uint32_t)(voc_mix(q.key + j++) >> 33);
      nd.first = (int)((double)r0 / (2147483647.0 + 1.0) * (double)q.n);
      for (int r = 1; r < k; r++) {
        uint32_t v;
        do {
          v = (uint32_t)(voc_mix(q.key + j++) >> 33);
        } while (v == 0);
        draws.push_back(v);
      }
      for (int i = 0; i < nd.n_items; i++)
        items.push_back(VtItem{(int)nodes.size(), q.start + i * kItem, std::min(kItem, q.n - i * kItem)});
      nodes.push_back(nd);
      keys.push_back(q.key);
      tnode_of.push_back(q.tnode);
    }
    const int nn = (int)nodes.size(), ni = (int)items.size(), nm = (int)multi_node.size();
    if (nn == 0) break;
    stats.n_kmeans_nodes += nn;

    DevBuf<VtNode> d_nodes(nn);
    DevBuf<VtItem> d_items(ni);
    DevBuf<uint32_t> d_draws(draws.size()), d_cent((size_t)nn * k * 8), d_item_sum(ni);
    DevBuf<uint32_t> d_gcnt((size_t)nm * k * 256), d_gsize((size_t)nm * k);
    DevBuf<int> d_ncent(nn), d_multi(nm), d_flags(2 * ((size_t)nn + 1));
    DevBuf<int> d_item_cnt((size_t)ni * k), d_item_off((size_t)ni * k), d_csize((size_t)nn * k);
    d_nodes.up(nodes, st);
    d_items.up(items, st);
    d_draws.up(draws, st);
    d_multi.up(multi_node, st);
    MMT_HIP(hipMemsetAsync(d_cent.p, 0, d_cent.n * 4, st));
    MMT_HIP(hipMemsetAsync(d_gcnt.p, 0, d_gcnt.n * 4, st));
    MMT_HIP(hipMemsetAsync(d_gsize.p, 0, d_gsize.n * 4, st));
    MMT_HIP(hipMemsetAsync(d_min.p, 0xFF, 4 * (size_t)N, st));
    MMT_HIP(hipMemsetAsync(d_assign.p, 0xFF, (size_t)N, st));

    // initiateClustersKMpp
    hipLaunchKernelGGL(k_seed_first, dim3((nn * 8 + 255) / 256), dim3(256), 0, st, d_nodes.p, nn, k,
                       d_desc.p, perm, d_cent.p, d_ncent.p);
    for (int r = 1; r < k; r++) {
      hipLaunchKernelGGL(k_seed_dist, dim3(ni), dim3(256), 0, st, d_items.p, d_desc.p, perm,
                         d_cent.p, d_ncent.p, k, d_min.p, d_item_sum.p);
      hipLaunchKernelGGL(k_seed_pick, dim3(nn), dim3(64), 0, st, d_nodes.p, r, k, d_draws.p,
                         d_item_sum.p, d_items.p, d_min.p, d_desc.p, perm, d_cent.p, d_ncent.p);
    }
    MMT_HIP(hipGetLastError());

    // Lloyd iterations of the whole level until no node's assignment changes.  flags: two blocks
    // of nn "changed" words plus the level's "some assignment changed" word.
    int* fl_prev = d_flags.p;
    int* fl_cur = d_flags.p + nn + 1;
    MMT_HIP(hipMemsetAsync(fl_prev, 0x01, 4 * ((size_t)nn + 1), st));  // every node is active
    int pass = 0;
    for (;;) {
      pass++;
      MMT_HIP(hipMemsetAsync(fl_cur, 0, 4 * ((size_t)nn + 1), st));
      if (pass > 1) {
        hipLaunchKernelGGL(k_vote, dim3(ni), dim3(256), 0, st, d_items.p, d_nodes.p, fl_prev,
                           d_desc.p, perm, d_assign.p, d_ncent.p, k, d_cent.p, d_gcnt.p, d_gsize.p);
        if (nm > 0)
          hipLaunchKernelGGL(k_means_multi, dim3(nm), dim3(256), 0, st, d_multi.p, fl_prev,
                             d_ncent.p, k, d_cent.p, d_gcnt.p, d_gsize.p);
      }
      hipLaunchKernelGGL(k_assign, dim3(ni), dim3(256), 0, st, d_items.p, fl_prev, d_desc.p, perm,
                         d_cent.p, d_ncent.p, k, d_assign.p, fl_cur, fl_cur + nn);
      MMT_HIP(hipGetLastError());
      int any = 0;
      MMT_HIP(hipMemcpyAsync(&any, fl_cur + nn, 4, hipMemcpyDeviceToHost, st));
      MMT_HIP(hipStreamSynchronize(st));
      if (!any) break;
      if (pass >= max_iters) {  // nodes still changing at the cap stop here
        h_changed.resize(nn);
        MMT_HIP(hipMemcpyAsync(h_changed.data(), fl_cur, 4 * (size_t)nn, hipMemcpyDeviceToHost, st));
        MMT_HIP(hipStreamSynchronize(st));
        for (int c : h_changed) stats.n_capped += c != 0;
        break;
      }
      std::swap(fl_prev, fl_cur);
    }
    stats.iters[level - 1] = pass;

    // groups: the stable partition of every segment by cluster
    hipLaunchKernelGGL(k_count, dim3(ni), dim3(64), 0, st, d_items.p, d_assign.p, k, d_item_cnt.p);
    hipLaunchKernelGGL(k_offsets, dim3((nn + 255) / 256), dim3(256), 0, st, d_nodes.p, nn, k,
                       d_item_cnt.p, d_item_off.p, d_csize.p);
    MMT_HIP(hipMemcpyAsync(perm2, perm, 4 * (size_t)N, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_scatter, dim3(ni), dim3(64), 0, st, d_items.p, d_nodes.p, d_assign.p, k,
                       d_item_off.p, perm, perm2);
    MMT_HIP(hipGetLastError());
    std::swap(perm, perm2);
    h_ncent.resize(nn);
    h_cent.resize((size_t)nn * k * 8);
    h_csize.resize((size_t)nn * k);
    d_ncent.down(h_ncent.data(), h_ncent.size(), st);
    d_cent.down(h_cent.data(), h_cent.size(), st);
    d_csize.down(h_csize.data(), h_csize.size(), st);
    MMT_HIP(hipMemcpyAsync(h_perm.data(), perm, 4 * (size_t)N, hipMemcpyDeviceToHost, st));
    MMT_HIP(hipStreamSynchronize(st));

    for (int n = 0; n < nn; n++) {
      int start = nodes[n].start;
      for (int c = 0; c < h_ncent[n]; c++) {
        const int sz = h_csize[(size_t)n * k + c];
        const int id = add_child(tnode_of[n], (const uint8_t*)&h_cent[((size_t)n * k + c) * 8]);
        if (sz == 0) stats.n_empty_clusters++;
        if (sz > 1 && level < L) next.push_back(Pending{id, start, sz, voc_mix(keys[n] ^ (uint64_t)(c + 1))});
        start += sz;
      }
    }
    pending.swap(next);
  }

  // ids as HKmeansStep assigns them: a node's children contiguous, then each child's subtree in
  // child order
  const int total = (int)t_parent.size();
  std::vector<int> parent(total, -1), new_id(total, 0);
  std::vector<uint8_t> descs(32 * (size_t)total, 0);
  {
    int next_id = 1;
    std::vector<std::pair<int, int>> stack{{0, 0}};  // (node, next child to descend into)
    for (int c = 0; c < t_nchild[0]; c++) new_id[t_first[0] + c] = next_id++;
    while (!stack.empty()) {
      auto& top = stack.back();
      if (top.second >= t_nchild[top.first]) {
        stack.pop_back();
        continue;
      }
      const int c = t_first[top.first] + top.second++;
      for (int g = 0; g < t_nchild[c]; g++) new_id[t_first[c] + g] = next_id++;
      stack.push_back({c, 0});
    }
  }
  for (int t = 1; t < total; t++) {
    parent[new_id[t]] = new_id[t_parent[t]];
    memcpy(&descs[32 * (size_t)new_id[t]], &t_desc[32 * (size_t)t], 32);
  }
  out.set_tree(k, L, p.scoring, p.weighting, parent, descs);
  stats.n_nodes = out.n_nodes();
  stats.n_words = out.n_words();

  // setNodeWeights: every training descriptor through the finished tree
  std::vector<double> w(out.n_words(), 1.0);
  if (p.weighting == 0 || p.weighting == 2) {
    out.upload();
    DevBuf<uint32_t> d_word(N), d_node(N);
    DevBuf<double> d_w(N);
    launch_bow_transform(out.dev, (const uint8_t*)d_desc.p, N, 0, d_word.p, d_w.p, d_node.p, st);
    std::vector<uint32_t> word(N);
    d_word.down(word.data(), word.size(), st);
    MMT_HIP(hipStreamSynchronize(st));
    std::vector<int> Ni(out.n_words(), 0), last(out.n_words(), -1);
    for (int im = 0; im < n_images; im++)
      for (int i = image_start[im]; i < image_start[im + 1]; i++)
        if (last[word[i]] != im) {
          last[word[i]] = im;
          Ni[word[i]]++;
        }
    for (int i = 0; i < out.n_words(); i++)
      w[i] = Ni[i] > 0 ? std::log((double)n_images / (double)Ni[i]) : 0.0;
  }
  out.set_word_weights(w);
}

}  // namespace mmt
