// scikit-learn's k-means for MANY recordings in one launch (include/sd_hip_kmeans.h, sd_kmeans_grouped_f64): one workgroup per
// (recording, restart), every phase on all 256 threads, f64 throughout; a second small launch selects among the restarts.  DESIGN.md
// section 23 has the argument.
//
//   (a) centre        the column means (thread (s, j) adds column j of the rows s, s + S, ...; S = 256 / dim slices, reduced in slice
//                     order), the rows minus them into LDS when they fit (column j of row i at j (n | 1) + i), the tolerance from
//                     the column variances.  A NaN or inf anywhere ends the restart with a flag.
//   (b) seed          greedy k-means++: `closest` in the workspace (a row belongs to the thread tid = i mod 256 in every phase that
//                     writes it), per step a block prefix sum of it, 256 rows at a time with a running carry, in which every thread
//                     counts for each trial the prefixes below v_j; the t candidates' rows go to LDS, every thread adds the t
//                     potentials over its rows, the best trial becomes the centre.
//   (c) Lloyd         a row per thread: the argmin over the centres in LDS, the label compared with the one before, an integer count
//                     per cluster; then thread (s, j) adds column j of its slice of rows into partial sums of its own,
//                     part[s][label][j]; thread (c, j) adds the S partial sums in slice order, divides, and squares the shift.
//   (d) the inertia, the iteration count and the flags of the restart go to the workspace.
//
// The rows are read through one accessor (LDS, or global memory minus the mean: the same bits), and every squared distance through
// one function with explicit fused multiply-adds, so a distance has one value wherever it is taken.  Every sum runs in an order
// that depends on (n, dim, k) alone.  Nothing is read from first_row, k or first and used as an address before it is compared with
// its range.
#include <hip/hip_runtime.h>

#include "sd_common.h"
#include "kmeans/sd_kmeans_check.h"
#include "sd_hip_kmeans.h"

namespace {

constexpr int KM_THREADS = SD_KM_THREADS;
constexpr int KM_TRIALS = SD_KM_TRIALS;
static_assert(SD_KMEANS_U_STRIDE == (SD_KM_MAX_K - 1) * SD_KM_TRIALS, "the draws of one restart");

// The recording's rows, centred: LDS when they fit, global memory otherwise
struct KmRows {
  const double* lds;      // null: streamed
  const double* glob;     // the recording's first row
  const double* mean;     // LDS
  long ld;
  int stride;             // n | 1
  __device__ __forceinline__ double operator()(const int i, const int j) const {
    return lds ? lds[j * stride + i] : glob[(long)i * ld + j] - mean[j];
  }
};

// |X_i - c|^2, c: dim doubles in LDS
__device__ __forceinline__ double km_dist2(const KmRows& X, const int i, const double* c, const int dim) {
  double acc = 0.0;
  for (int j = 0; j < dim; ++j) {
    const double diff = X(i, j) - c[j];
    acc = fma(diff, diff, acc);
  }
  return acc;
}

// The sum of v over the 256 threads, in every thread: a fixed tree inside the wave, the four waves in order.  s_red: 4 doubles of LDS.
// Called by every thread; two barriers, the first of which lets the readers of the last call finish.
__device__ __forceinline__ double km_block_sum(double v, double* s_red) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

// The inclusive prefix sum of v over the 256 threads, and the sum of all of them in *total.  Same calling rules as km_block_sum.
__device__ __forceinline__ double km_scan(const double v, double* s_red, double* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const double up = __shfl_up(inc, d);
    if (lane >= d) inc += up;
  }
  __syncthreads();
  if (lane == 63) s_red[wave] = inc;
  __syncthreads();
  double before = 0.0, sum = 0.0;
  for (int w = 0; w < KM_THREADS / 64; ++w) {
    const double t = s_red[w];
    before += w < wave ? t : 0.0;
    sum += t;
  }
  *total = sum;
  return before + inc;
}

__device__ __forceinline__ bool km_finite(const double v) { return ((__double2hiint(v) >> 20) & 0x7ff) != 0x7ff; }

// The promise about first_row, all of it, by every thread of the workgroup: the label ranges and the slices of the workspace are
// disjoint only under it.  s_bad: one int of LDS, 0 on entry.
__device__ __forceinline__ bool km_promise_broken(const int* __restrict__ first_row, const int n_groups, const int n_rows, int* s_bad) {
  for (int i = threadIdx.x; i <= n_groups; i += KM_THREADS) {
    const int fr = first_row[i];
    bool broken = fr < 0 || fr > n_rows || (i == 0 && fr != 0) || (i == n_groups && fr != n_rows);
    if (i < n_groups) broken |= first_row[i + 1] < fr;
    if (broken) *s_bad = 1;                                      // every thread that finds it stores the same 1
  }
  __syncthreads();
  const bool broken = *s_bad != 0;
  __syncthreads();                                               // everyone has read it before anyone stores to it again
  return broken;
}

struct KmArgs {
  const double* rows;
  long ld;
  int n_rows, dim;
  const int* first_row;
  int n_groups;
  const int* k;
  int n_init, max_iter, max_k;
  double tol_rel;
  const int* first;
  const double* u;
  double* closest;        // [n_init][n_rows]
  double* r_inertia;      // [n_groups][n_init]
  int* r_labels;          // [n_init][n_rows]
  int* r_iters;           // [n_groups][n_init]
  int* r_flags;           // [n_groups][n_init]
  int rows_cap;           // doubles of LDS for the rows
};

__global__ __launch_bounds__(KM_THREADS) void kmeans_lloyd_kernel(const KmArgs a) {
  extern __shared__ __attribute__((aligned(16))) double km_lds[];
  __shared__ double s_red[4];
  __shared__ double s_tol;
  __shared__ int s_cnt[SD_KM_MAX_K];
  __shared__ int s_trial[KM_TRIALS];
  __shared__ int s_bad, s_changed, s_empty;
  const int tid = threadIdx.x, dim = a.dim;
  const int g = blockIdx.x / a.n_init, r = blockIdx.x % a.n_init, slot = g * a.n_init + r;
  if (tid == 0) s_bad = 0, s_changed = 0, s_empty = 0;
  __syncthreads();
  if (km_promise_broken(a.first_row, a.n_groups, a.n_rows, &s_bad)) return;      // the selection flags every recording
  const int r0 = a.first_row[g], n = a.first_row[g + 1] - r0;     // 0 <= r0, r0 + n <= n_rows, disjoint from every other recording's
  const int k = a.k[g], f = a.first[slot];
  int flags = (k < 2 || k > a.max_k || k >= n) ? SD_KMEANS_BAD_K : 0;
  if (!flags && (f < 0 || f >= n)) flags = SD_KMEANS_BAD_DRAW;
  if (flags) {                                                   // workgroup-uniform
    if (tid == 0) a.r_flags[slot] = flags, a.r_iters[slot] = 0, a.r_inertia[slot] = 0.0;
    return;
  }

  // ---- the layout of LDS (sd_kmeans_check.h): centres, partial sums, means, candidates, rows
  const int S = sd_km_slices(dim);
  double* const s_centre = km_lds;
  double* const s_part = s_centre + a.max_k * dim;
  double* const s_mean = s_part + S * a.max_k * dim;
  double* const s_cand = s_mean + dim;
  double* const s_rows = s_cand + KM_TRIALS * dim;
  const int stride = n | 1;
  const bool in_lds = (long)dim * stride <= (long)a.rows_cap;
  const double* const mine = a.rows + (long)r0 * a.ld;
  const int ps = tid / dim, pj = tid % dim;                      // the slice and the column of this thread in the column-wise phases
  const bool p_on = ps < S;
  double* const closest = a.closest + (long)r * a.n_rows + r0;
  int* const lab = a.r_labels + (long)r * a.n_rows + r0;

  // ---- (a) the column means; every value looked at
  {
    double acc = 0.0;
    bool finite = true;
    if (p_on)
      for (int i = ps; i < n; i += S) {
        const double v = mine[(long)i * a.ld + pj];
        finite &= km_finite(v);
        acc += v;
      }
    if (!finite) s_bad = 1;
    if (p_on) s_part[ps * dim + pj] = acc;
    __syncthreads();
    if (tid < dim) {
      double sum = 0.0;
      for (int s = 0; s < S; ++s) sum += s_part[s * dim + tid];
      s_mean[tid] = sum / (double)n;
    }
    __syncthreads();
    if (s_bad) {                                                 // workgroup-uniform
      if (tid == 0) a.r_flags[slot] = SD_KMEANS_NONFINITE, a.r_iters[slot] = 0, a.r_inertia[slot] = 0.0;
      return;
    }
    if (in_lds && p_on)
      for (int i = ps; i < n; i += S) s_rows[pj * stride + i] = mine[(long)i * a.ld + pj] - s_mean[pj];
    __syncthreads();
  }
  KmRows X;
  X.lds = in_lds ? s_rows : nullptr, X.glob = mine, X.mean = s_mean, X.ld = a.ld, X.stride = stride;
  {                                                              // the tolerance: tol_rel x the mean of the column variances
    double acc = 0.0;
    if (p_on)
      for (int i = ps; i < n; i += S) {
        const double v = X(i, pj);
        acc = fma(v, v, acc);
      }
    if (p_on) s_part[ps * dim + pj] = acc;
    __syncthreads();
    if (tid == 0) {
      double all = 0.0;
      for (int j = 0; j < dim; ++j) {
        double sum = 0.0;
        for (int s = 0; s < S; ++s) sum += s_part[s * dim + j];
        all += sum / (double)n;
      }
      s_tol = a.tol_rel == 0.0 ? 0.0 : a.tol_rel * (all / (double)dim);
    }
    __syncthreads();
  }
  const double tol = s_tol;

  // ---- (b) greedy k-means++
  const int t = k < 3 ? 2 : k < 8 ? 3 : k < 21 ? 4 : 5;          // 2 + floor(ln k) for 2 <= k <= 32
  if (tid < dim) s_centre[tid] = X(f, tid);
  __syncthreads();
  double pot;
  {
    double acc = 0.0;
    for (int i = tid; i < n; i += KM_THREADS) {
      const double d = km_dist2(X, i, s_centre, dim);
      closest[i] = d;
      acc += d;
    }
    pot = km_block_sum(acc, s_red);
  }
  for (int c = 1; c < k; ++c) {
    const double* const uc = a.u + ((long)slot * (SD_KM_MAX_K - 1) + (c - 1)) * KM_TRIALS;
    double v[KM_TRIALS];
    int below[KM_TRIALS];
#pragma unroll
    for (int j = 0; j < KM_TRIALS; ++j) v[j] = j < t ? uc[j] * pot : 0.0, below[j] = 0;
    if (tid < KM_TRIALS) s_trial[tid] = 0;
    double carry = 0.0;
    for (int base = 0; base < n; base += KM_THREADS) {           // base is uniform: every thread reaches the scan
      const int i = base + tid;
      double total;
      const double prefix = carry + km_scan(i < n ? closest[i] : 0.0, s_red, &total);
      if (i < n) {
#pragma unroll
        for (int j = 0; j < KM_TRIALS; ++j) below[j] += prefix < v[j] ? 1 : 0;
      }
      carry += total;
    }
#pragma unroll
    for (int j = 0; j < KM_TRIALS; ++j)
      if (j < t && below[j]) atomicAdd(&s_trial[j], below[j]);   // after the scans' barriers: s_trial was zeroed before them
    __syncthreads();
    if (tid < t * dim) {
      const int j = tid / dim, cand = s_trial[j] < n - 1 ? s_trial[j] : n - 1;     // a count of rows: 0 <= cand < n
      s_cand[tid] = X(cand, tid % dim);
    }
    __syncthreads();
    double acc[KM_TRIALS];
#pragma unroll
    for (int j = 0; j < KM_TRIALS; ++j) acc[j] = 0.0;
    for (int i = tid; i < n; i += KM_THREADS) {
      const double cl = closest[i];
#pragma unroll
      for (int j = 0; j < KM_TRIALS; ++j)
        if (j < t) acc[j] += fmin(cl, km_dist2(X, i, s_cand + j * dim, dim));
    }
    int best = 0;
    double best_pot = 0.0;
#pragma unroll
    for (int j = 0; j < KM_TRIALS; ++j)
      if (j < t) {                                               // t is uniform: every thread reaches the sums
        const double p = km_block_sum(acc[j], s_red);
        if (j == 0 || p < best_pot) best = j, best_pot = p;
      }
    if (tid < dim) s_centre[c * dim + tid] = s_cand[best * dim + tid];
    for (int i = tid; i < n; i += KM_THREADS) closest[i] = fmin(closest[i], km_dist2(X, i, s_cand + best * dim, dim));
    pot = best_pot;
    __syncthreads();                                             // s_cand and s_trial are free again
  }

  // ---- (c) Lloyd
  for (int i = tid; i < n; i += KM_THREADS) lab[i] = -1;
  int iters = 0;
  bool strict = false;
  for (int it = 1; it <= a.max_iter; ++it) {
    if (tid == 0) s_changed = 0;
    if (tid < k) s_cnt[tid] = 0;
    for (int p = tid; p < S * k * dim; p += KM_THREADS) s_part[p] = 0.0;
    __syncthreads();
    for (int i = tid; i < n; i += KM_THREADS) {
      int arg = 0;
      double least = km_dist2(X, i, s_centre, dim);
      for (int c = 1; c < k; ++c) {
        const double d = km_dist2(X, i, s_centre + c * dim, dim);
        if (d < least) least = d, arg = c;
      }
      if (lab[i] != arg) s_changed = 1;                          // every thread that finds it stores the same 1
      lab[i] = arg;
      atomicAdd(&s_cnt[arg], 1);
    }
    __syncthreads();
    const bool changed = s_changed != 0;
    if (p_on)
      for (int i = ps; i < n; i += S) s_part[(ps * k + lab[i]) * dim + pj] += X(i, pj);      // 0 <= lab[i] < k: written above
    if (tid < k && s_cnt[tid] == 0) s_empty = 1;
    __syncthreads();
    double moved = 0.0;
    for (int p = tid; p < k * dim; p += KM_THREADS) {
      const int c = p / dim, j = p % dim;
      double sum = 0.0;
      for (int s = 0; s < S; ++s) sum += s_part[(s * k + c) * dim + j];
      const double centre = sum / (double)s_cnt[c];
      const double diff = centre - s_centre[p];
      s_centre[p] = centre;
      moved = fma(diff, diff, moved);
    }
    const double shift = km_block_sum(moved, s_red);             // its barriers publish the centres and s_empty
    if (s_empty) {                                               // workgroup-uniform
      if (tid == 0) a.r_flags[slot] = SD_KMEANS_EMPTY, a.r_iters[slot] = it, a.r_inertia[slot] = 0.0;
      return;
    }
    iters = it;
    if (!changed) {
      strict = true;
      break;
    }
    if (shift <= tol) break;
  }
  double acc = 0.0;
  for (int i = tid; i < n; i += KM_THREADS) {
    int arg = lab[i];
    if (!strict) {                                               // the labels once more, against the final centres
      arg = 0;
      double least = km_dist2(X, i, s_centre, dim);
      for (int c = 1; c < k; ++c) {
        const double d = km_dist2(X, i, s_centre + c * dim, dim);
        if (d < least) least = d, arg = c;
      }
      lab[i] = arg;
    }
    acc += km_dist2(X, i, s_centre + arg * dim, dim);
  }
  const double inertia = km_block_sum(acc, s_red);
  if (tid == 0) a.r_flags[slot] = 0, a.r_iters[slot] = iters, a.r_inertia[slot] = inertia;
}

// The selection among the restarts of a recording, in restart order, and the copy of the chosen labels: one workgroup per recording.
__global__ __launch_bounds__(KM_THREADS) void kmeans_select_kernel(const int* __restrict__ first_row, const int n_groups, const int n_rows,
                                                                   const int* __restrict__ ks, const int n_init,
                                                                   const double* __restrict__ r_inertia, const int* __restrict__ r_labels,
                                                                   const int* __restrict__ r_iters, const int* __restrict__ r_flags,
                                                                   int* __restrict__ labels, int* __restrict__ chosen,
                                                                   double* __restrict__ inertia, int* __restrict__ iters, int* __restrict__ flags) {
  __shared__ int s_map[SD_KM_MAX_K];
  __shared__ int s_bad, s_differ;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_bad = 0, s_differ = 0;
  __syncthreads();
  if (km_promise_broken(first_row, n_groups, n_rows, &s_bad)) {   // no recording has a range of its own: every workgroup fills its share with -1
    const long from = (long)n_rows * g / n_groups, to = (long)n_rows * (g + 1) / n_groups;
    for (long p = from + tid; p < to; p += KM_THREADS) labels[p] = -1;
    if (tid == 0) flags[g] = SD_KMEANS_BAD_PROMISE, chosen[g] = -1, inertia[g] = 0.0, iters[g] = 0;
    return;
  }
  const int r0 = first_row[g], n = first_row[g + 1] - r0;
  int* const out = labels + r0;
  int all = 0;
  for (int r = 0; r < n_init; ++r) all |= r_flags[g * n_init + r];
  if (all) {                                                     // workgroup-uniform
    for (int i = tid; i < n; i += KM_THREADS) out[i] = -1;
    if (tid == 0) flags[g] = all, chosen[g] = -1, inertia[g] = 0.0, iters[g] = 0;
    return;
  }
  const int k = ks[g];                                           // 2 <= k <= 32: the restarts checked it, and their labels lie in [0, k)
  int best = 0;
  for (int r = 1; r < n_init; ++r) {
    if (!(r_inertia[g * n_init + r] < r_inertia[g * n_init + best])) continue;       // uniform
    if (tid < k) s_map[tid] = -1;
    if (tid == 0) s_differ = 0;
    __syncthreads();
    const int* const mine = r_labels + (long)r * n_rows + r0;
    const int* const theirs = r_labels + (long)best * n_rows + r0;
    for (int i = tid; i < n; i += KM_THREADS) {
      const int to = theirs[i], was = atomicCAS(&s_map[mine[i]], -1, to);
      if (was != -1 && was != to) s_differ = 1;
    }
    __syncthreads();
    const bool differ = s_differ != 0;
    __syncthreads();                                             // everyone has read it before the next restart resets it
    if (differ) best = r;
  }
  const int* const from = r_labels + (long)best * n_rows + r0;
  for (int i = tid; i < n; i += KM_THREADS) out[i] = from[i];
  if (tid == 0) flags[g] = 0, chosen[g] = best, inertia[g] = r_inertia[g * n_init + best], iters[g] = r_iters[g * n_init + best];
}

}  // namespace

extern "C" int sd_kmeans_abi_version(void) { return SD_KMEANS_ABI_VERSION; }

extern "C" size_t sd_kmeans_grouped_workspace_bytes(int n_rows, int n_groups, int n_init) {
  return sd_kmeans_workspace_bytes(n_rows, n_groups, n_init);
}

extern "C" int sd_kmeans_grouped_f64(const double* rows, long ld, int n_rows, int dim, const int* first_row, int n_groups, const int* k, int n_init,
                                     int max_iter, double tol_rel, int max_k, int max_rows, const int* first, const double* u, int* labels,
                                     int* chosen, double* inertia, int* iters, int* flags, void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SdKmeansCall c = {};
  c.n_rows = n_rows, c.dim = dim, c.n_groups = n_groups, c.n_init = n_init, c.max_iter = max_iter, c.max_k = max_k, c.max_rows = max_rows;
  c.ld = ld, c.tol_rel = tol_rel;
  c.table_null = !(first_row && k && first && u && chosen && inertia && iters && flags && ws);
  c.rows_null = !(rows && labels);
  c.rows_misaligned = (reinterpret_cast<uintptr_t>(rows) & 7u) != 0;
  c.ws_misaligned = !sd_aligned16(ws);
  c.ws_bytes = ws_bytes;
  char why[SD_KMEANS_WHY];
  if (const int e = sd_kmeans_check(c, why)) return sd_set_error(e, "%s", why);
  KmArgs a;
  a.rows = rows, a.ld = ld, a.n_rows = n_rows, a.dim = dim, a.first_row = first_row, a.n_groups = n_groups, a.k = k, a.n_init = n_init;
  a.max_iter = max_iter, a.max_k = max_k, a.tol_rel = tol_rel, a.first = first, a.u = u;
  const size_t per_restart = (size_t)n_init * (size_t)n_rows, slots = (size_t)n_init * (size_t)n_groups;
  a.closest = static_cast<double*>(ws);
  a.r_inertia = a.closest + per_restart;
  a.r_labels = reinterpret_cast<int*>(a.r_inertia + slots);
  a.r_iters = a.r_labels + per_restart;
  a.r_flags = a.r_iters + slots;
  a.rows_cap = sd_km_rows_cap(dim, max_k, max_rows);
  const size_t lds = (size_t)8 * ((size_t)sd_km_fixed_doubles(dim, max_k) + (size_t)a.rows_cap);
  SD_CHECK_HIP(sd_func_max_lds(reinterpret_cast<const void*>(kmeans_lloyd_kernel), SD_KM_LDS_BYTES - SD_KM_LDS_STATIC));   // set once: the most any launch asks for
  hipLaunchKernelGGL(kmeans_lloyd_kernel, dim3((unsigned)(n_groups * n_init)), dim3(KM_THREADS), lds, stream, a);
  SD_CHECK_LAUNCH("kmeans_lloyd_kernel");
  hipLaunchKernelGGL(kmeans_select_kernel, dim3((unsigned)n_groups), dim3(KM_THREADS), 0, stream, first_row, n_groups, n_rows, k, n_init,
                     a.r_inertia, a.r_labels, a.r_iters, a.r_flags, labels, chosen, inertia, iters, flags);
  SD_CHECK_LAUNCH("kmeans_select_kernel");
  return SD_OK;
}
