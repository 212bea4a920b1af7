// From the merge log of the AHC driver to the labels at a bounded cluster count, for MANY recordings in one launch
// (include/sd_hip_cut.h, sd_ahc_cut_grouped): one workgroup per recording, every phase on all 256 threads.  DESIGN.md section 22 has
// the argument.
//
//   (a) check, count   every merge of the recording: lo < hi inside [0, n_g), a finite key; c = the merges with key > cos_thr.
//                      m = max(0, min(max(c, n_g - max), n_g - min)) is workgroup-uniform.
//   (b) select         the m-th smallest 64-bit composite (inverted order-preserving key bits, position): a radix select, 8 passes of
//                      8 bits from the top, each a 256-bin histogram in LDS over the merges that match the digits found so far.  The
//                      merges are read from global memory again in every pass: nothing is sized by the recording.
//   (c) scatter        parent[row] = row, a barrier, parent[hi] = lo for every merge whose composite is at most the selected one, a
//                      barrier, and every such merge reads parent[hi] again: another lo there means two parents for one row.
//   (d) roots          every row walks to its root (at most n_g steps; parent[x] < x for every x that is no root) and keeps it in
//                      `labels`.
//   (e) ranks          a prefix sum over the flags parent[row] == row, 256 rows at a time, gives every root its rank, stored over
//                      parent[root]; a row's label is the rank of its root.
//
// Nothing is read from lo, hi, first_merge or first_row and used as an address before it is compared with its range.
#include <hip/hip_runtime.h>

#include "sd_common.h"
#include "cut/sd_cut_check.h"
#include "sd_hip_cut.h"

namespace {

constexpr int CT_THREADS = 256;
typedef unsigned long long ct_u64;

// (key, position) as one integer that ascends where the order (key descending, position ascending) does; -0.0 counts as 0.0
__device__ __forceinline__ ct_u64 ct_composite(const float key, const int pos) {
  unsigned bits = __float_as_uint(key);
  if (bits == 0x80000000u) bits = 0;
  const unsigned ascending = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  return ((ct_u64)(~ascending) << 32) | (unsigned)pos;
}

// The exclusive prefix sum of v over the 256 threads, and the sum of all of them in *total.  s_w: 4 words of LDS.  Called by every
// thread of the workgroup; two barriers, the first of which lets the readers of the last call finish.
__device__ __forceinline__ int ct_scan(const int v, int* s_w, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc, d);
    if (lane >= d) inc += up;
  }
  __syncthreads();
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int before = 0, sum = 0;
  for (int w = 0; w < CT_THREADS / 64; ++w) {
    const int t = s_w[w];
    before += w < wave ? t : 0;
    sum += t;
  }
  *total = sum;
  return before + inc - v;
}

__global__ __launch_bounds__(CT_THREADS) void ahc_cut_grouped_kernel(const int* __restrict__ lo, const int* __restrict__ hi,
                                                                     const float* __restrict__ key, const int* __restrict__ first_merge,
                                                                     const int* __restrict__ first_row, const int n_groups, const int n_merges,
                                                                     const int n_rows, const float cos_thr, const int* __restrict__ min_clusters,
                                                                     const int* __restrict__ max_clusters, int* labels, int* __restrict__ clusters,
                                                                     int* __restrict__ bad, int* parent_all) {
  __shared__ int s_hist[256];
  __shared__ int s_w[CT_THREADS / 64];
  __shared__ int s_bad, s_count, s_bucket, s_k;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_bad = 0, s_count = 0;
  __syncthreads();

  // the promise about first_merge and first_row, all of it: the label ranges and the slices of `parent` are disjoint only under it
  for (int i = tid; i <= n_groups; i += CT_THREADS) {
    const int fm = first_merge[i], fr = first_row[i];
    bool broken = fm < 0 || fm > n_merges || fr < 0 || fr > n_rows || (i == 0 && (fm != 0 || fr != 0)) ||
                  (i == n_groups && (fm != n_merges || fr != n_rows));
    if (i < n_groups) broken |= first_merge[i + 1] < fm || first_row[i + 1] < fr;
    if (broken) s_bad = 1;                                       // every thread that finds it stores the same 1
  }
  __syncthreads();
  const bool promise_broken = s_bad != 0;
  __syncthreads();                                               // everyone has read s_bad before anyone stores to it again
  if (promise_broken) {                                          // no recording has a range of its own: every workgroup fills its share with -1
    const long from = (long)n_rows * g / n_groups, to = (long)n_rows * (g + 1) / n_groups;
    for (long p = from + tid; p < to; p += CT_THREADS) labels[p] = -1;
    if (tid == 0) bad[g] = 1, clusters[g] = 0;
    return;
  }
  const int a = first_merge[g], L = first_merge[g + 1] - a;      // 0 <= a, a + L <= n_merges
  const int r0 = first_row[g], n = first_row[g + 1] - r0;        // 0 <= r0, r0 + n <= n_rows, disjoint from every other recording's
  int* const out = labels + r0;
  int* const parent = parent_all + r0;
  const int mn = min_clusters[g], mx = max_clusters[g];
  bool refused = mn < 1 || mn > mx || L > (n > 1 ? n - 1 : 0);   // workgroup-uniform, as everything `refused` takes below

  // ---- (a) every merge checked, and the count above the threshold
  if (!refused) {
    int mine = 0;
    for (int i = tid; i < L; i += CT_THREADS) {
      const int x = lo[a + i], y = hi[a + i];
      const float k = key[a + i];
      if (x < 0 || x >= y || y >= n || ((__float_as_uint(k) >> 23) & 0xffu) == 0xffu) s_bad = 1;
      mine += k > cos_thr ? 1 : 0;
    }
    if (mine) atomicAdd(&s_count, mine);
  }
  __syncthreads();
  refused |= s_bad != 0;
  int m = 0;
  if (!refused) {
    const int c = s_count, at_most = n - mx, at_least = n - mn;  // n >= 0 and 1 <= mn <= mx: no overflow
    m = c > at_most ? c : at_most;
    m = m < at_least ? m : at_least;
    m = m > 0 ? m : 0;
    refused = m > L;                                             // the log is too short for the maximum
  }

  // ---- (b) the m-th smallest composite
  ct_u64 cutoff = 0;
  const bool select = !refused && m > 0;
  if (select) {
    int k = m;
    for (int shift = 56; shift >= 0; shift -= 8) {
      s_hist[tid] = 0;                                           // CT_THREADS == 256 bins
      __syncthreads();
      for (int i = tid; i < L; i += CT_THREADS) {
        const ct_u64 comp = ct_composite(key[a + i], i);
        if (shift == 56 || (comp >> (shift + 8)) == cutoff) atomicAdd(&s_hist[(int)((comp >> shift) & 255u)], 1);
      }
      __syncthreads();
      const int h = s_hist[tid];
      int total;
      const int before = ct_scan(h, s_w, &total);
      if (before < k && k <= before + h) s_bucket = tid, s_k = k - before;      // one thread: 1 <= k <= total
      __syncthreads();
      cutoff = (cutoff << 8) | (unsigned)s_bucket;
      k = s_k;
    }
  }

  // ---- (c) the forest
  for (int p = tid; p < n; p += CT_THREADS) parent[p] = p;
  __syncthreads();
  if (select) {
    for (int i = tid; i < L; i += CT_THREADS)
      if (ct_composite(key[a + i], i) <= cutoff) parent[hi[a + i]] = lo[a + i];             // checked in (a): 0 <= lo < hi < n
    __syncthreads();
    for (int i = tid; i < L; i += CT_THREADS)
      if (ct_composite(key[a + i], i) <= cutoff && parent[hi[a + i]] != lo[a + i]) s_bad = 1;   // another merge took this row
    __syncthreads();
    refused |= s_bad != 0;
  }

  if (refused) {
    for (int p = tid; p < n; p += CT_THREADS) out[p] = -1;
    if (tid == 0) bad[g] = 1, clusters[g] = 0;
    return;
  }

  // ---- (d) every row to its root: parent holds checked values of lo (below the row) or the row itself
  for (int p = tid; p < n; p += CT_THREADS) {
    int r = p;
    for (int steps = 0; steps < n; ++steps) {
      const int up = parent[r];
      if (up == r) break;
      r = up;
    }
    out[p] = r;
  }
  __syncthreads();

  // ---- (e) the rank of every root among the roots, over parent[root]; then the labels
  int roots = 0;
  for (int base = 0; base < n; base += CT_THREADS) {             // base is uniform: every thread reaches the scan
    const int p = base + tid;
    const int flag = p < n && parent[p] == p ? 1 : 0;
    int total;
    const int before = ct_scan(flag, s_w, &total);
    if (flag) parent[p] = roots + before;                        // rows of later tiles are not touched; no walk runs any more
    roots += total;
  }
  __syncthreads();
  for (int p = tid; p < n; p += CT_THREADS) out[p] = parent[out[p]];
  if (tid == 0) bad[g] = 0, clusters[g] = n - m;
}

}  // namespace

extern "C" int sd_cut_abi_version(void) { return SD_CUT_ABI_VERSION; }

extern "C" size_t sd_ahc_cut_workspace_bytes(int n_rows, int n_groups) { return sd_cut_workspace_bytes(n_rows, n_groups); }

extern "C" int sd_ahc_cut_grouped(const int* lo, const int* hi, const float* key, const int* first_merge, const int* first_row, int n_groups,
                                  int n_merges, int n_rows, float cos_thr, const int* min_clusters, const int* max_clusters, int* labels,
                                  int* clusters, int* bad, void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SdCutCall c = {};
  c.n_groups = n_groups, c.n_merges = n_merges, c.n_rows = n_rows, c.cos_thr = cos_thr;
  c.table_null = !(first_merge && first_row && min_clusters && max_clusters && clusters && bad);
  c.merges_null = !(lo && hi && key);
  c.rows_null = labels == nullptr;
  c.ws_null = ws == nullptr;
  c.ws_misaligned = !sd_aligned16(ws);
  c.ws_bytes = ws_bytes;
  char why[SD_CUT_WHY];
  if (const int e = sd_cut_check(c, why)) return sd_set_error(e, "%s", why);
  hipLaunchKernelGGL(ahc_cut_grouped_kernel, dim3((unsigned)n_groups), dim3(CT_THREADS), 0, stream, lo, hi, key, first_merge, first_row, n_groups,
                     n_merges, n_rows, cos_thr, min_clusters, max_clusters, labels, clusters, bad, static_cast<int*>(ws));
  SD_CHECK_LAUNCH("ahc_cut_grouped_kernel");
  return SD_OK;
}
