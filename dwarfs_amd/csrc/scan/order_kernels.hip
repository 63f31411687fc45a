// Nilsimsa fragment ordering (src/writer/internal/similarity_ordering.cpp of the reference): the two
// distance loops of --order=nilsimsa on the device, and the whole algorithm restated on the host.
//
//   split   cluster_by_distance for every node of one tree level: one workgroup per node walks the node's
//           elements in list order (each add changes a centroid, so the walk is serial); inside a step the
//           lanes take the node's children kSplitThreads at a time, a min-reduction finds the lowest child
//           with distance <= max_distance (the scan stops after the pass that holds it), a (distance, index)
//           min-reduction serves the full node, 256 lanes update the 256 bit counters and four ballots
//           rebuild the centroid's four words.  Centroids, counters and member counts live in the caller's
//           workspace: a node with m elements owns min(m, max_children) child slots from its base on.
//   chain   order_by_shortest_path for every segment: one workgroup per segment, the permutation and the
//           256-bit rows in LDS when the segment has at most kStageRows entries, in global memory otherwise.
//           A step is a (class, k) min-reduction with class = 0 for d <= 1 and d above, which is the
//           sequential rule "the first k with d <= 1, else the first arg-min"; then one swap.
//
// No workgroup waits on another; a level's dependence on the level before is a launch boundary.  Every loop
// is bounded by a count read once from the launch's arrays.  No 64-bit shift takes a variable amount.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "ricepp_amd.h"

namespace {

constexpr int kSplitThreads = 1024;     // children per pass of the split
constexpr int kChainThreads = 256;      // entries per pass of the chain
constexpr uint32_t kStageRows = 896;    // 2 x 32 B rows + 4 B permutation entry each: 60928 B of LDS
constexpr uint32_t kBad = 0xffffffffu;
constexpr uint64_t kNone = ~0ull;

__device__ inline uint64_t wave_min_u64(uint64_t v) {
  for (int o = 32; o; o >>= 1) {
    const uint64_t t = (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}

// The minimum over the workgroup, returned to every thread, with one barrier: the two halves of `red`
// alternate, and a half is rewritten only after the barrier of the call in between, which no thread
// passes before it has read the half.  Every thread of the workgroup makes every call.
template <int Threads>
__device__ inline uint64_t block_min_u64(uint64_t v, uint64_t (*red)[Threads / 64], uint32_t& parity) {
  v = wave_min_u64(v);
  if ((threadIdx.x & 63) == 0) red[parity][threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t r = red[parity][0];
#pragma unroll
  for (int w = 1; w < Threads / 64; ++w) {
    const uint64_t t = red[parity][w];
    r = t < r ? t : r;
  }
  parity ^= 1;
  return r;
}

__device__ inline uint32_t distance4(const uint64_t* a, uint64_t b0, uint64_t b1, uint64_t b2, uint64_t b3) {
  const ulonglong2 lo = *reinterpret_cast<const ulonglong2*>(a);
  const ulonglong2 hi = *reinterpret_cast<const ulonglong2*>(a + 2);
  return __popcll(lo.x ^ b0) + __popcll(lo.y ^ b1) + __popcll(hi.x ^ b2) + __popcll(hi.y ^ b3);
}

__global__ __launch_bounds__(kSplitThreads) void rpp_order_split_kernel(
    const uint64_t* __restrict__ bits, uint32_t n_elems, const uint32_t* __restrict__ index,
    const uint32_t* __restrict__ node_start, const uint64_t* __restrict__ child_base, uint64_t slots,
    uint32_t max_children, uint32_t max_distance, uint32_t* __restrict__ child_out,
    uint32_t* __restrict__ nchildren_out, uint64_t* cent, uint32_t* counts, uint32_t* members) {
  __shared__ uint64_t red[2][kSplitThreads / 64];
  uint32_t parity = 0;
  const uint32_t node = blockIdx.x, t = threadIdx.x;
  const uint32_t s0 = node_start[node];
  const uint32_t m = node_start[node + 1] - s0;
  const uint64_t base = child_base[node];
  if (base > slots || (m < max_children ? m : max_children) > slots - base) {  // (the same for every thread)
    if (t == 0) nchildren_out[node] = kBad;
    return;
  }
  uint64_t* const C = cent + 4 * base;
  uint32_t* const K = counts + 256 * base;
  uint32_t* const V = members + base;
  uint32_t nch = 0;

  // element e's words and element e + 1's id are in registers when step e starts
  uint32_t id = m ? index[s0] : 0, id_next = m > 1 ? index[s0 + 1] : 0;
  uint64_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
  if (m && id < n_elems) {
    const uint64_t* v = bits + 4 * (uint64_t)id;
    v0 = v[0], v1 = v[1], v2 = v[2], v3 = v[3];
  }
  for (uint32_t e = 0; e < m; ++e) {
    if (id >= n_elems) {  // (every thread holds the same id)
      if (t == 0) nchildren_out[node] = kBad;
      return;
    }
    uint64_t n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    if (e + 1 < m && id_next < n_elems) {
      const uint64_t* v = bits + 4 * (uint64_t)id_next;
      n0 = v[0], n1 = v[1], n2 = v[2], n3 = v[3];
    }
    const uint32_t id_next2 = e + 2 < m ? index[s0 + e + 2] : 0;

    uint64_t found = kNone, best = kNone;
    for (uint32_t c0 = 0; c0 < nch; c0 += kSplitThreads) {
      const uint32_t c = c0 + t;
      uint64_t key = kNone;
      if (c < nch) {
        const uint32_t d = distance4(C + 4 * (uint64_t)c, v0, v1, v2, v3);
        if (d <= max_distance) {
          key = c;
        } else {
          const uint64_t k = ((uint64_t)d << 32) | c;
          best = k < best ? k : best;  // (c ascends per thread: the earliest child keeps a tie)
        }
      }
      found = block_min_u64<kSplitThreads>(key, red, parity);
      if (found != kNone) break;
    }
    uint32_t chosen;
    bool fresh = false;
    if (found != kNone) {
      chosen = (uint32_t)found;
    } else if (nch < max_children) {
      chosen = nch++;
      fresh = true;
    } else {
      chosen = (uint32_t)block_min_u64<kSplitThreads>(best, red, parity);
    }

    // centroid.add: counter t and centroid bit t belong to thread t, wave w rebuilds word w
    const uint64_t vw = t < 64 ? v0 : t < 128 ? v1 : t < 192 ? v2 : v3;
    const uint32_t half = (t & 32) ? (uint32_t)(vw >> 32) : (uint32_t)vw;
    const uint32_t bit = (half >> (t & 31)) & 1;
    if (fresh) {
      if (t < 256) K[256 * (uint64_t)chosen + t] = bit;
      if (t == 0) {
        C[4 * (uint64_t)chosen] = v0, C[4 * (uint64_t)chosen + 1] = v1;
        C[4 * (uint64_t)chosen + 2] = v2, C[4 * (uint64_t)chosen + 3] = v3;
        V[chosen] = 1;
      }
    } else {
      const uint32_t vc = V[chosen] + 1;
      __syncthreads();  // every thread has read the member count
      if (t == 0) V[chosen] = vc;
      if (t < 256) {
        const uint32_t cnt = K[256 * (uint64_t)chosen + t] + bit;
        K[256 * (uint64_t)chosen + t] = cnt;
        const uint64_t word = __ballot(cnt > vc / 2);
        if ((t & 63) == 0) C[4 * (uint64_t)chosen + (t >> 6)] = word;
      }
    }
    if (t == 0) child_out[s0 + e] = chosen;
    __syncthreads();  // the step's stores are visible to the next step's loads
    id = id_next, id_next = id_next2;
    v0 = n0, v1 = n1, v2 = n2, v3 = n3;
  }
  if (t == 0) nchildren_out[node] = nch;
}

__global__ __launch_bounds__(kChainThreads) void rpp_order_chain_kernel(
    const uint64_t* __restrict__ bits, uint32_t n_elems, const uint32_t* __restrict__ from_ids,
    const uint32_t* __restrict__ to_ids, const uint32_t* __restrict__ seg_start, uint32_t* perm_out) {
  __shared__ __attribute__((aligned(16))) uint64_t s_to[kStageRows * 4];
  __shared__ __attribute__((aligned(16))) uint64_t s_from[kStageRows * 4];
  __shared__ uint32_t s_perm[kStageRows];
  __shared__ uint64_t red[2][kChainThreads / 64];
  uint32_t parity = 0;
  const uint32_t t = threadIdx.x;
  const uint32_t s0 = seg_start[blockIdx.x];
  const uint32_t count = seg_start[blockIdx.x + 1] - s0;
  const bool same = from_ids == to_ids;

  int bad = 0;
  for (uint32_t k = t; k < count; k += kChainThreads) bad |= from_ids[s0 + k] >= n_elems || to_ids[s0 + k] >= n_elems;
  if (__syncthreads_or(bad)) {
    for (uint32_t k = t; k < count; k += kChainThreads) perm_out[s0 + k] = kBad;
    return;
  }
  const bool staged = count <= kStageRows;
  if (staged) {
    for (uint32_t k = t; k < count; k += kChainThreads) {
      const uint64_t* r = bits + 4 * (uint64_t)to_ids[s0 + k];
      s_to[4 * k] = r[0], s_to[4 * k + 1] = r[1], s_to[4 * k + 2] = r[2], s_to[4 * k + 3] = r[3];
      if (!same) {
        const uint64_t* f = bits + 4 * (uint64_t)from_ids[s0 + k];
        s_from[4 * k] = f[0], s_from[4 * k + 1] = f[1], s_from[4 * k + 2] = f[2], s_from[4 * k + 3] = f[3];
      }
      s_perm[k] = k;
    }
  } else {
    for (uint32_t k = t; k < count; k += kChainThreads) perm_out[s0 + k] = k;
  }
  __syncthreads();
  uint32_t* const P = staged ? s_perm : perm_out + s0;  // the permutation in progress: original positions
  const uint64_t* const F = same ? s_to : s_from;

  for (uint32_t i = 0; i + 1 < count; ++i) {
    const uint32_t pi = P[i];
    const uint64_t* fr = staged ? F + 4 * pi : bits + 4 * (uint64_t)from_ids[s0 + pi];
    const uint64_t f0 = fr[0], f1 = fr[1], f2 = fr[2], f3 = fr[3];
    uint64_t best = kNone, r = kNone;
    for (uint32_t k0 = i + 1; k0 < count; k0 += kChainThreads) {
      const uint32_t k = k0 + t;
      if (k < count && k >= k0) {
        const uint32_t pk = P[k];
        const uint64_t* row = staged ? s_to + 4 * pk : bits + 4 * (uint64_t)to_ids[s0 + pk];
        const uint32_t d = distance4(row, f0, f1, f2, f3);
        const uint64_t key = ((uint64_t)(d <= 1 ? 0 : d) << 32) | k;
        best = key < best ? key : best;
      }
      r = block_min_u64<kChainThreads>(best, red, parity);
      if ((r >> 32) == 0) break;  // a d <= 1 in this pass: the sequential scan stops there
      if (k0 + kChainThreads < k0) break;
    }
    const uint32_t bk = (uint32_t)r;
    if (t == 0 && bk != i + 1) {
      const uint32_t a = P[i + 1];
      P[i + 1] = P[bk];
      P[bk] = a;
    }
    __syncthreads();
  }
  if (staged)
    for (uint32_t k = t; k < count; k += kChainThreads) perm_out[s0 + k] = s_perm[k];
}

int launched() { return hipGetLastError() == hipSuccess ? RPP_OK : RPP_HIP_ERROR; }

uint64_t align16(uint64_t v) { return (v + 15) & ~15ull; }

// ---- the host restatement: the reference's sequential algorithm, nothing shared with the kernels ----

struct View {
  const uint64_t* bits;
  const uint64_t* sizes;
  const uint32_t* rank;  // NULL: the element's own number
  uint32_t rk(uint32_t a) const { return rank ? rank[a] : a; }
  const uint64_t* row(uint32_t a) const { return bits + 4 * (size_t)a; }
  bool bits_equal(uint32_t a, uint32_t b) const { return memcmp(row(a), row(b), 32) == 0; }
  bool bitvec_less(uint32_t a, uint32_t b) const {
    for (int i = 0; i < 4; ++i)
      if (row(a)[i] != row(b)[i]) return row(a)[i] < row(b)[i];
    return rk(a) < rk(b);
  }
  bool order_less(uint32_t a, uint32_t b) const {
    if (sizes[a] != sizes[b]) return sizes[a] > sizes[b];
    return rk(a) < rk(b);
  }
};

int host_distance(const uint64_t* a, const uint64_t* b) {
  int d = 0;
  for (int i = 0; i < 4; ++i) d += __builtin_popcountll(a[i] ^ b[i]);
  return d;
}

struct Centroid {
  uint64_t value[4] = {0, 0, 0, 0};
  uint32_t bitcounts[256] = {};
  uint32_t veccount = 0;
  void add(const uint64_t* vec) {
    ++veccount;
    for (int bit = 0; bit < 256; ++bit) {
      bitcounts[bit] += (vec[bit / 64] >> (bit % 64)) & 1;
      if (bitcounts[bit] > veccount / 2)
        value[bit / 64] |= 1ull << (bit % 64);
      else
        value[bit / 64] &= ~(1ull << (bit % 64));
    }
  }
};

struct Cluster {
  Centroid centroid;
  std::vector<uint32_t> index;
};

struct Node {
  std::vector<uint32_t> index;  // a leaf's elements
  std::vector<Node> children;
  bool leaf = true;
  uint32_t first() const { return leaf ? index.front() : children.front().first(); }
  uint32_t last() const { return leaf ? index.back() : children.back().last(); }
};

template <typename From, typename To, typename Swap>
void host_chain(size_t count, const From& from, const To& to, const Swap& swapper, uint64_t* early) {
  for (size_t i = 0; i + 1 < count; ++i) {
    const uint64_t* bi = from(i);
    int best_distance = 0x7fffffff;
    size_t best_index = 0;
    for (size_t k = i + 1; k < count; ++k) {
      const int d = host_distance(bi, to(k));
      if (d < best_distance) {
        best_distance = d;
        best_index = k;
        if (best_distance <= 1) {
          if (early) ++*early;
          break;
        }
      }
    }
    if (best_index > 0 && i + 1 != best_index) swapper(i + 1, best_index);
  }
}

struct HostOrder {
  View ev;
  uint32_t max_children, max_cluster_size;
  rpp_order_stats st{};

  // cluster_by_distance: `list` in visiting order -> clusters in creation order; child[e] (when given) is
  // the cluster element e of the list went to
  std::vector<Cluster> split(const std::vector<uint32_t>& list, int max_distance, uint32_t* child) {
    std::vector<Cluster> children;
    for (size_t e = 0; e < list.size(); ++e) {
      const uint64_t* vec = ev.row(list[e]);
      size_t match = SIZE_MAX, best_match = SIZE_MAX;
      int best_distance = 0x7fffffff;
      bool tie = false;
      for (size_t c = 0; c < children.size(); ++c) {
        const int d = host_distance(children[c].centroid.value, vec);
        if (d <= max_distance) {
          match = c;
          break;
        }
        if (d < best_distance) {
          best_distance = d;
          best_match = c;
          tie = false;
        } else if (d == best_distance) {
          tie = true;
        }
      }
      if (match == SIZE_MAX) {
        if (children.size() < max_children) {
          children.emplace_back();
          match = children.size() - 1;
        } else {
          match = best_match;
          ++st.fallbacks;
          if (tie) ++st.fallback_ties;
        }
      }
      children[match].centroid.add(vec);
      children[match].index.push_back(list[e]);
      if (child) child[e] = (uint32_t)match;
    }
    return children;
  }

  void order_cluster(std::vector<uint32_t>& index) {
    std::sort(index.begin(), index.end(), [this](uint32_t a, uint32_t b) { return ev.order_less(a, b); });
    host_chain(
        index.size(), [&](size_t i) { return ev.row(index[i]); }, [&](size_t k) { return ev.row(index[k]); },
        [&](size_t i, size_t k) { std::swap(index[i], index[k]); }, &st.chain_early_stops);
  }

  void cluster_rec(Node& node, int max_distance, uint32_t level) {
    st.depth = std::max(st.depth, level);
    std::vector<Cluster> clusters = split(node.index, max_distance, nullptr);
    st.largest_node = std::max<uint32_t>(st.largest_node, (uint32_t)clusters.size());
    node.leaf = false;
    node.index = {};
    node.children.resize(clusters.size());
    for (size_t c = 0; c < clusters.size(); ++c) {
      Node& cn = node.children[c];
      cn.index = std::move(clusters[c].index);
      if (max_distance > 1 && cn.index.size() > max_cluster_size) {
        cluster_rec(cn, max_distance / 2, level + 1);
        continue;
      }
      ++st.leaves;
      st.largest_leaf = std::max<uint32_t>(st.largest_leaf, (uint32_t)cn.index.size());
      if (max_distance == 1) st.largest_final_leaf = std::max<uint32_t>(st.largest_final_leaf, (uint32_t)cn.index.size());
      if (cn.index.size() > 1) order_cluster(cn.index);
    }
  }

  uint64_t order_tree_rec(Node& node) {
    if (node.leaf) {
      uint64_t w = 0;
      for (uint32_t i : node.index) w += ev.sizes[i];
      return w;
    }
    struct Entry {
      const uint64_t *first, *last;
      size_t child;
      uint64_t weight;
    };
    std::vector<Entry> entries;
    uint64_t total = 0;
    for (size_t c = 0; c < node.children.size(); ++c) {
      const uint64_t w = order_tree_rec(node.children[c]);
      entries.push_back({ev.row(node.children[c].first()), ev.row(node.children[c].last()), c, w});
      total += w;
    }
    std::stable_sort(entries.begin(), entries.end(), [](const Entry& a, const Entry& b) { return a.weight > b.weight; });
    host_chain(
        entries.size(), [&](size_t i) { return entries[i].last; }, [&](size_t k) { return entries[k].first; },
        [&](size_t i, size_t k) { std::swap(entries[i], entries[k]); }, &st.chain_early_stops);
    std::vector<Node> ordered;
    ordered.reserve(entries.size());
    for (const Entry& en : entries) ordered.push_back(std::move(node.children[en.child]));
    node.children.swap(ordered);
    return total;
  }

  void run(std::vector<uint32_t> index, uint32_t* out) {
    if (index.empty()) return;
    std::sort(index.begin(), index.end(), [this](uint32_t a, uint32_t b) { return ev.bitvec_less(a, b); });
    // duplicates: dup_of[k] lists what follows the k-th unique element
    std::vector<uint32_t> unique;
    std::vector<std::vector<uint32_t>> dups;
    for (uint32_t id : index) {
      if (!unique.empty() && ev.bits_equal(unique.back(), id)) {
        dups.back().push_back(id);
      } else {
        unique.push_back(id);
        dups.emplace_back();
      }
    }
    std::vector<uint32_t> slot_of;  // element id -> its place in `unique`, for the collect
    for (const auto& d : dups) st.duplicate_groups += !d.empty();
    st.unique = (uint32_t)unique.size();
    Node root;
    root.index = unique;
    cluster_rec(root, 128, 1);
    order_tree_rec(root);
    // collect: depth first in child order
    uint32_t max_id = *std::max_element(unique.begin(), unique.end());
    slot_of.assign((size_t)max_id + 1, 0);
    for (size_t k = 0; k < unique.size(); ++k) slot_of[unique[k]] = (uint32_t)k;
    size_t o = 0;
    std::vector<const Node*> stack{&root};
    while (!stack.empty()) {
      const Node* nd = stack.back();
      stack.pop_back();
      if (!nd->leaf) {
        for (size_t c = nd->children.size(); c--;) stack.push_back(&nd->children[c]);
        continue;
      }
      for (uint32_t e : nd->index) {
        out[o++] = e;
        std::vector<uint32_t>& dv = dups[slot_of[e]];
        std::sort(dv.begin(), dv.end(), [this](uint32_t a, uint32_t b) { return ev.order_less(a, b); });
        for (uint32_t i : dv) out[o++] = i;
      }
    }
  }
};

}  // namespace

extern "C" int rpp_order_check_options(uint32_t max_children, uint32_t max_cluster_size) {
  return max_children >= 1 && max_cluster_size >= 1 ? RPP_OK : RPP_UNSUPPORTED_CONFIG;
}

extern "C" uint32_t rpp_order_split_pass_children(void) { return kSplitThreads; }
extern "C" uint32_t rpp_order_chain_threads(void) { return kChainThreads; }
extern "C" uint32_t rpp_order_chain_stage_rows(void) { return kStageRows; }

extern "C" uint64_t rpp_order_split_workspace_bytes(uint64_t child_slots) {
  return align16(child_slots * 32) + align16(child_slots * 1024) + align16(child_slots * 4);
}

extern "C" uint64_t rpp_order_chain_workspace_bytes(uint64_t total_entries) {
  (void)total_entries;  // the permutation in progress of a segment beyond the LDS lives in the output itself
  return 0;
}

extern "C" int rpp_order_split_batch(const uint64_t* d_bits, uint32_t n_elems, const uint32_t* d_index,
                                     const uint32_t* d_node_start, const uint64_t* d_child_base, uint32_t n_nodes,
                                     uint64_t child_slots, uint32_t max_children, uint32_t max_distance,
                                     uint32_t* d_child, uint32_t* d_nchildren, void* d_workspace,
                                     uint64_t workspace_bytes, void* stream) {
  if (rpp_order_check_options(max_children, 1) != RPP_OK) return RPP_UNSUPPORTED_CONFIG;
  if (n_nodes == 0) return RPP_OK;
  if (!d_bits || !d_index || !d_node_start || !d_child_base || !d_child || !d_nchildren || !d_workspace ||
      max_distance > 256 || ((uintptr_t)d_workspace & 15) || ((uintptr_t)d_bits & 15) ||
      child_slots > (1ull << 40) || workspace_bytes < rpp_order_split_workspace_bytes(child_slots))
    return RPP_INVALID_ARGUMENT;
  uint8_t* ws = static_cast<uint8_t*>(d_workspace);
  uint64_t* cent = reinterpret_cast<uint64_t*>(ws);
  uint32_t* counts = reinterpret_cast<uint32_t*>(ws + align16(child_slots * 32));
  uint32_t* members = reinterpret_cast<uint32_t*>(ws + align16(child_slots * 32) + align16(child_slots * 1024));
  hipLaunchKernelGGL(rpp_order_split_kernel, dim3(n_nodes), dim3(kSplitThreads), 0, static_cast<hipStream_t>(stream),
                     d_bits, n_elems, d_index, d_node_start, d_child_base, child_slots, max_children, max_distance,
                     d_child, d_nchildren, cent, counts, members);
  return launched();
}

extern "C" int rpp_order_chain_batch(const uint64_t* d_bits, uint32_t n_elems, const uint32_t* d_from_ids,
                                     const uint32_t* d_to_ids, const uint32_t* d_seg_start, uint32_t n_segments,
                                     uint32_t* d_perm, void* stream) {
  if (n_segments == 0) return RPP_OK;
  if (!d_bits || !d_from_ids || !d_to_ids || !d_seg_start || !d_perm || ((uintptr_t)d_bits & 15))
    return RPP_INVALID_ARGUMENT;
  hipLaunchKernelGGL(rpp_order_chain_kernel, dim3(n_segments), dim3(kChainThreads), 0,
                     static_cast<hipStream_t>(stream), d_bits, n_elems, d_from_ids, d_to_ids, d_seg_start, d_perm);
  return launched();
}

extern "C" int rpp_order_host_split(const uint64_t* bits, uint32_t n_elems, const uint32_t* index, uint32_t m,
                                    uint32_t max_children, uint32_t max_distance, uint32_t* child,
                                    uint32_t* nchildren) {
  if (rpp_order_check_options(max_children, 1) != RPP_OK) return RPP_UNSUPPORTED_CONFIG;
  if (!bits || (m && (!index || !child)) || !nchildren || max_distance > 256) return RPP_INVALID_ARGUMENT;
  for (uint32_t e = 0; e < m; ++e)
    if (index[e] >= n_elems) return RPP_INVALID_ARGUMENT;
  HostOrder h{View{bits, nullptr, nullptr}, max_children, 1};
  *nchildren = (uint32_t)h.split(std::vector<uint32_t>(index, index + m), (int)max_distance, child).size();
  return RPP_OK;
}

extern "C" int rpp_order_host_chain(const uint64_t* bits, uint32_t n_elems, const uint32_t* from_ids,
                                    const uint32_t* to_ids, uint32_t count, uint32_t* perm) {
  if (!bits || (count && (!from_ids || !to_ids || !perm))) return RPP_INVALID_ARGUMENT;
  for (uint32_t k = 0; k < count; ++k)
    if (from_ids[k] >= n_elems || to_ids[k] >= n_elems) return RPP_INVALID_ARGUMENT;
  std::iota(perm, perm + count, 0u);
  host_chain(
      count, [&](size_t i) { return bits + 4 * (size_t)from_ids[perm[i]]; },
      [&](size_t k) { return bits + 4 * (size_t)to_ids[perm[k]]; },
      [&](size_t i, size_t k) { std::swap(perm[i], perm[k]); }, nullptr);
  return RPP_OK;
}

extern "C" int rpp_order_host_nilsimsa(const uint64_t* bits, const uint64_t* sizes, const uint32_t* rank,
                                       uint32_t n_elems, const uint32_t* index, uint32_t n_index,
                                       uint32_t max_children, uint32_t max_cluster_size, uint32_t* out,
                                       rpp_order_stats* stats) {
  if (rpp_order_check_options(max_children, max_cluster_size) != RPP_OK) return RPP_UNSUPPORTED_CONFIG;
  if (n_index && (!bits || !sizes || !index || !out)) return RPP_INVALID_ARGUMENT;
  for (uint32_t k = 0; k < n_index; ++k)
    if (index[k] >= n_elems) return RPP_INVALID_ARGUMENT;
  HostOrder h{View{bits, sizes, rank}, max_children, max_cluster_size};
  h.run(std::vector<uint32_t>(index, index + n_index), out);
  if (stats) *stats = h.st;
  return RPP_OK;
}
