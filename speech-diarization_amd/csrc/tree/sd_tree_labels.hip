// From a spanning tree's edges to HDBSCAN's labels for MANY recordings in one launch (include/sd_hip_tree.h, sd_tree_labels_grouped):
// one workgroup per recording.  The result is scikit-learn 1.7.2's `tree_to_labels(make_single_linkage(mst[order]), ...)` with
// order = argsort(dist, kind="stable"), exactly; DESIGN.md section 21 has the argument for every step.
//
//   (a) sort      all threads: a bitonic network over the positions of the edges, compared by (bits of dist, position).  The bits order
//                 as the values do for finite doubles >= 0 and the keys are distinct, so the result is the stable order.  The network
//                 is the one that sorts ascending in every stage (the first step of a merge mirrors its block): a partner past the
//                 last edge stands for +inf and is skipped, no padding is stored.
//   (b) dendrogram   one lane: union-find over 2 n - 1 nodes; edge i of the sorted list makes node n + i from the roots of its ends.
//   (c) condense, (d) stabilities   one lane: breadth-first from the root over the LIVE nodes (those not inside a pruned subtree).  A
//                 node whose two sides both hold min_cluster_size rows is a true split: its sides become clusters K and K + 1.  A side
//                 below min_cluster_size is pruned: its rows, in breadth-first order of the side, fall out of the node's cluster at the
//                 node's lambda.  Every entry of the condensed tree adds (lambda - birth of the parent) * size to the parent's
//                 stability the moment it is made, which is condensed-tree order; a row adds its term once, c rows c times.
//   (e) selection   one lane: clusters from the last to the first (children before parents): the two children's sum against the
//                 cluster's own stability with a strict >, then from the first to the last: a cluster stays selected when no ancestor
//                 is, and every cluster learns the label of the rows that fall out of it.
//   (f) labels    all threads: a row takes the label of the cluster of the node it fell out at; under a single selected root, 0 when
//                 its lambda reaches the largest lambda of the root's own entries.
//
// The state (sd_tree_check.h has the bytes) is addressed through one base pointer: LDS when the recording's rows fit, its slice of
// the workspace otherwise.  Nothing is read from lo, hi or first_edge and used as an address before it is compared with its range;
// every loop is bounded by the recording's size and sets `bad` instead of going on.
#include <hip/hip_runtime.h>

#include "sd_common.h"
#include "tree/sd_tree_check.h"
#include "sd_hip_tree.h"

// a stability is a sum of separately rounded products: no fused multiply-add anywhere in this file
#pragma clang fp contract(off)

namespace {

constexpr int TL_THREADS = 256;
typedef unsigned long long tl_u64;

// lambda of a distance given by its bits: 1 / dist by IEEE division, +inf for 0
__device__ __forceinline__ double tl_lambda(const tl_u64 bits) {
  const double d = __longlong_as_double((long long)bits);
  return d > 0.0 ? 1.0 / d : (double)INFINITY;
}

struct TlState {
  tl_u64* key;       // [m] the bits of dist, by position in the list
  double* stab;      // [K] stabilities
  int* ord;          // [m] the sorted order: position in the list of the i-th smallest edge
  int* left;         // [m] dendrogram: node n + i joins left[i] and right[i] and has csize[i] rows
  int* right;
  int* csize;
  int* ufp;          // [2 n] union-find parent (-1: a root); after (b) the queue of a pruned subtree
  int* mainq;        // [m] lo of every edge until (b) is done; then the queue of live nodes
  int* ncl;          // [m] hi of every edge until (b) is done; then the cluster of a live node
  int* pnode;        // [n] the node a row fell out at
  int* cparent;      // [K] parent cluster
  int* fchild;       // [K] first of the two child clusters, -1 for none; after (e) the label of the rows that fall out of the cluster
  int* cnode;        // [K] the node whose split made the cluster (its birth), -1 for the root; after (e) whether an ancestor-or-self is selected
  int* sel;          // [K] selected
};

__device__ __forceinline__ TlState tl_carve(unsigned char* base, const int n) {
  TlState s;
  s.key = reinterpret_cast<tl_u64*>(base);
  s.stab = reinterpret_cast<double*>(base + (size_t)8 * n);
  int* w = reinterpret_cast<int*>(base + (size_t)16 * n);
  s.ord = w, s.left = w + n, s.right = w + 2 * (size_t)n, s.csize = w + 3 * (size_t)n, s.ufp = w + 4 * (size_t)n;
  s.mainq = w + 6 * (size_t)n, s.ncl = w + 7 * (size_t)n, s.pnode = w + 8 * (size_t)n, s.cparent = w + 9 * (size_t)n;
  s.fchild = w + 10 * (size_t)n, s.cnode = w + 11 * (size_t)n, s.sel = w + 12 * (size_t)n;       // 13 n ints of the 14 n
  return s;
}

// the root of x, with path compression; -1 when the walk runs out of its bound of 2 n steps
__device__ __forceinline__ int tl_find(int* __restrict__ ufp, int x, const int n) {
  int r = x, steps = 0;
  while (ufp[r] >= 0) {
    r = ufp[r];
    if (++steps > 2 * n) return -1;
  }
  for (int s = 0; s < steps; ++s) {
    const int up = ufp[x];
    ufp[x] = r;
    x = up;
  }
  return r;
}

// (b) to (e) on one lane -> 0, or 1 when the edges are not a spanning tree or a bound ran out.  *thr: the largest lambda among the
// entries of the root cluster
__device__ int tl_sequential(const TlState& s, const int n, const int m, const int mcs, const int allow_single, double* thr_out) {
  // ---- (b) the dendrogram
  for (int i = 0; i < m; ++i) {
    const int e = s.ord[i];
    const int rx = tl_find(s.ufp, s.mainq[e], n), ry = tl_find(s.ufp, s.ncl[e], n);
    if (rx < 0 || ry < 0 || rx == ry) return 1;                 // an edge inside one component: not a tree
    s.left[i] = rx, s.right[i] = ry;
    s.csize[i] = (rx >= n ? s.csize[rx - n] : 1) + (ry >= n ? s.csize[ry - n] : 1);
    s.ufp[rx] = s.ufp[ry] = n + i;
  }
  // n - 1 unions of distinct components over n rows: one component, node 2 n - 2 is the root

  // ---- (c), (d) condense breadth-first over the live nodes; the stabilities as the entries are made
  int* const subq = s.ufp;
  int K = 1, head = 0, tail = 1;
  double thr = -(double)INFINITY;
  s.cparent[0] = -1, s.fchild[0] = -1, s.cnode[0] = -1, s.stab[0] = 0.0;
  s.ncl[m - 1] = 0, s.mainq[0] = m - 1;
  while (head < tail) {                                          // tail <= m: every node is queued at most once
    const int h = s.mainq[head++];
    const int c = s.ncl[h];
    const int L = s.left[h], R = s.right[h];
    const int lc = L >= n ? s.csize[L - n] : 1, rc = R >= n ? s.csize[R - n] : 1;
    const double lam = tl_lambda(s.key[s.ord[h]]);
    const int born = s.cnode[c];
    const double term = lam - (born < 0 ? 0.0 : tl_lambda(s.key[s.ord[born]]));
    if (c == 0 && lam > thr) thr = lam;
    double st = s.stab[c];
    if (lc >= mcs && rc >= mcs) {                                // a true split: two clusters, numbered left before right
      if (K + 2 > n || tail + 2 > m) return 1;
      const int cl = K, cr = K + 1;
      K += 2;
      s.fchild[c] = cl;
      s.cparent[cl] = s.cparent[cr] = c;
      s.cnode[cl] = s.cnode[cr] = h;
      s.fchild[cl] = s.fchild[cr] = -1;
      s.stab[cl] = s.stab[cr] = 0.0;
      st = st + term * (double)lc;
      st = st + term * (double)rc;
      s.ncl[L - n] = cl, s.ncl[R - n] = cr;
      s.mainq[tail++] = L - n, s.mainq[tail++] = R - n;
    } else {
      for (int side = 0; side < 2; ++side) {
        const int top = side ? R : L, count = side ? rc : lc;
        if (count >= mcs) {                                      // the cluster goes on down this side
          if (tail + 1 > m) return 1;
          s.ncl[top - n] = c;
          s.mainq[tail++] = top - n;
          continue;
        }
        int sh = 0, st_ = 1;                                     // pruned: its rows fall out here, breadth-first
        subq[0] = top;
        while (sh < st_) {                                       // st_ <= 2 count - 1 < 2 n
          const int v = subq[sh++];
          if (v < n) {
            s.pnode[v] = h;
            st = st + term;
          } else {
            if (st_ + 2 > 2 * n) return 1;
            subq[st_++] = s.left[v - n];
            subq[st_++] = s.right[v - n];
          }
        }
      }
    }
    s.stab[c] = st;
  }

  // ---- (e) excess of mass: children before parents; the root is a candidate only with allow_single
  for (int c = K - 1; c >= (allow_single ? 0 : 1); --c) {
    const int fc = s.fchild[c];
    double sub = 0.0;
    if (fc >= 0) {
      sub = sub + s.stab[fc];
      sub = sub + s.stab[fc + 1];
    }
    if (sub > s.stab[c]) {
      s.sel[c] = 0;
      s.stab[c] = sub;
    } else {
      s.sel[c] = 1;
    }
  }
  if (!allow_single) s.sel[0] = 0;
  // parents before children: a cluster under a selected one is not selected; the label of a selected cluster is its rank among the
  // selected ids, -2 stands for a selected root (then the only one: the rule of (f)), -1 for no selected ancestor-or-self
  int* const code = s.fchild;
  int* const covered = s.cnode;
  int n_sel = 0;
  for (int c = 0; c < K; ++c) {
    const int par = s.cparent[c];
    const int above = c == 0 ? 0 : covered[par];
    const int up = c == 0 ? -1 : code[par];
    if (s.sel[c] && !above) {
      code[c] = c == 0 ? -2 : n_sel;
      ++n_sel;
      covered[c] = 1;
    } else {
      code[c] = above ? up : -1;
      covered[c] = above;
    }
  }
  *thr_out = thr;
  return 0;
}

__global__ __launch_bounds__(TL_THREADS) void tree_labels_grouped_kernel(const int* __restrict__ lo, const int* __restrict__ hi,
                                                                         const tl_u64* __restrict__ dist, const int* __restrict__ first_edge,
                                                                         const int n_groups, const int n_edges, const int max_edges,
                                                                         const int mcs, const int allow_single, int* __restrict__ labels,
                                                                         int* __restrict__ bad, unsigned char* __restrict__ ws,
                                                                         const int lds_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char tl_lds[];
  __shared__ int s_bad;
  __shared__ double s_thr;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_bad = 0;
  __syncthreads();

  // the promise about first_edge, all of it: the label ranges and the workspace slices are disjoint only under it
  for (int i = tid; i <= n_groups; i += TL_THREADS) {
    const int v = first_edge[i];
    bool broken = v < 0 || v > n_edges || (i == 0 && v != 0) || (i == n_groups && v != n_edges);
    if (i < n_groups) broken |= first_edge[i + 1] < v;
    if (broken) s_bad = 1;                                       // every thread that finds it stores the same 1
  }
  __syncthreads();
  const bool promise_broken = s_bad != 0;
  __syncthreads();                                               // everyone has read s_bad before anyone stores to it again
  if (promise_broken) {                                          // no recording has a range of its own: every workgroup fills its share with -1
    const long total = (long)n_edges + n_groups;
    const long from = total * g / n_groups, to = total * (g + 1) / n_groups;
    for (long p = from + tid; p < to; p += TL_THREADS) labels[p] = -1;
    if (tid == 0) bad[g] = 1;
    return;
  }
  const int a = first_edge[g], b = first_edge[g + 1];            // 0 <= a <= b <= n_edges, disjoint from every other recording's
  const int m = b - a, n = m + 1;
  int* const out = labels + (size_t)a + g;                       // a + g + n <= n_edges + n_groups
  if (m < 1 || m > max_edges) {                                  // workgroup-uniform
    for (int p = tid; p < n; p += TL_THREADS) out[p] = -1;
    if (tid == 0) bad[g] = 1;
    return;
  }

  const TlState s = tl_carve(n <= lds_rows ? tl_lds : ws + (size_t)SD_TREE_ROW_BYTES * ((size_t)a + g), n);

  // the edges into the state, each checked: both ends rows of the recording, the distance finite and >= 0
  for (int i = tid; i < m; i += TL_THREADS) {
    const int x = lo[a + i], y = hi[a + i];
    tl_u64 bits = dist[a + i];
    if (bits == 0x8000000000000000ull) bits = 0;                 // -0.0 is 0
    if ((unsigned)x >= (unsigned)n || (unsigned)y >= (unsigned)n || (bits >> 63) || ((bits >> 52) & 0x7ff) == 0x7ff) s_bad = 1;
    s.key[i] = bits;
    s.ord[i] = i;
    s.mainq[i] = x, s.ncl[i] = y;
  }
  for (int i = tid; i < 2 * n - 1; i += TL_THREADS) s.ufp[i] = -1;
  for (int i = tid; i < n; i += TL_THREADS) s.pnode[i] = -1;
  __syncthreads();
  const bool refused = s_bad != 0;
  __syncthreads();                                               // as above: lane 0 stores to s_bad below

  if (!refused) {                                                // workgroup-uniform
    // ---- (a) the sort
    unsigned P = 1;
    while (P < (unsigned)m) P <<= 1;
    for (unsigned k = 2; k <= P && k != 0; k <<= 1) {                  // k != 0: P = 2^31 does not wrap the loop round
      for (unsigned j = k >> 1; j >= 1; j >>= 1) {
        const bool mirror = j == k >> 1;                         // the first step of a merge compares i with its mirror image in the block
        for (unsigned t = tid; t < P >> 1; t += TL_THREADS) {
          const unsigned l = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const unsigned p = mirror ? (l | (k - 1)) - (t & (j - 1)) : l + j;
          if (p < (unsigned)m) {
            const int ea = s.ord[l], eb = s.ord[p];
            const tl_u64 ka = s.key[ea], kb = s.key[eb];
            if (ka > kb || (ka == kb && ea > eb)) s.ord[l] = eb, s.ord[p] = ea;
          }
        }
        __syncthreads();
      }
    }
    // ---- (b) to (e)
    if (tid == 0) {
      double thr = 0.0;
      if (tl_sequential(s, n, m, mcs, allow_single, &thr)) s_bad = 1;
      s_thr = thr;
    }
  }
  __syncthreads();

  // ---- (f)
  const bool failed = s_bad != 0;
  const double thr = s_thr;
  for (int p = tid; p < n; p += TL_THREADS) {
    int label = -1;
    const int h = failed ? -1 : s.pnode[p];
    if (h >= 0) {
      label = s.fchild[s.ncl[h]];
      if (label == -2) label = tl_lambda(s.key[s.ord[h]]) >= thr ? 0 : -1;
    }
    out[p] = label;
  }
  if (tid == 0) bad[g] = failed ? 1 : 0;
}

}  // namespace

extern "C" int sd_tree_abi_version(void) { return SD_TREE_ABI_VERSION; }

extern "C" size_t sd_tree_labels_workspace_bytes(int n_edges, int n_groups, int max_edges) {
  return sd_tree_workspace_bytes(n_edges, n_groups, max_edges);
}

extern "C" int sd_tree_labels_grouped(const int* lo, const int* hi, const double* dist, const int* first_edge, int n_groups, int n_edges,
                                      int max_edges, int min_cluster_size, int allow_single_cluster, int* labels, int* bad, void* ws,
                                      size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SdTreeCall c = {n_edges, n_groups, max_edges, min_cluster_size, allow_single_cluster};
  c.any_null = !(lo && hi && dist && first_edge && labels && bad);
  c.ws_null = ws == nullptr;
  c.dist_misaligned = (reinterpret_cast<uintptr_t>(dist) & 7u) != 0;
  c.ws_misaligned = !sd_aligned16(ws);
  c.ws_bytes = ws_bytes;
  char why[SD_TREE_WHY];
  if (const int e = sd_tree_check(c, why)) return sd_set_error(e, "%s", why);
  const int lds_rows = sd_tree_lds_rows(max_edges);
  const int lds_bytes = lds_rows * SD_TREE_ROW_BYTES;
  SD_CHECK_HIP(sd_func_max_lds(reinterpret_cast<const void*>(tree_labels_grouped_kernel), SD_TREE_LDS_ROWS * SD_TREE_ROW_BYTES));     // set once: the most any launch asks for
  hipLaunchKernelGGL(tree_labels_grouped_kernel, dim3((unsigned)n_groups), dim3(TL_THREADS), (size_t)lds_bytes, stream, lo, hi,
                     reinterpret_cast<const tl_u64*>(dist), first_edge, n_groups, n_edges, max_edges, min_cluster_size, allow_single_cluster,
                     labels, bad, static_cast<unsigned char*>(ws), lds_rows);
  SD_CHECK_LAUNCH("tree_labels_grouped_kernel");
  return SD_OK;
}
