// Speaker-change detection for the segments of MANY recordings at once (include/sd_hip_scd.h): the window embeddings of a segment to
// its split pieces.  DESIGN.md section 25 has the argument.
//
// scd_split_kernel      a workgroup owns a segment of n rows, m = n - 1 distances.
//   (a) cosines         a wave takes the pairs w, w + 4, ... through sd_wave_pair_cosine (sd_common.h: the device code of
//                       sd_adjacent_cosine_f32, so the bits are its bits); d = 1.f - s goes to the distance list
//   (b) statistics      mean and population std of the distances in f64, two passes, an order fixed by m (sc_sum)
//   (c) peaks           256 distances at a time: "a run of equal values starts here" -> the start l of every run by a block scan with
//                       the operator max; a run that ends in a fall and started in a rise is a peak at (l + r) / 2; a prefix sum
//                       ranks the peaks whose z reaches thr, and each stores its cut at its rank
//   (d) chain           every thread finds next(j) of its cuts by binary search (rule 7 is monotone in the cut); thread 0 walks the
//                       chain and stores the pieces
// The distances, the cuts and the chain live in LDS up to SD_SCD_LDS_ROWS rows and in the segment's slice of `ws` above that.
//
// Contraction: the whole file is compiled with `fp contract(off)` (the pragma below; sd_wave_pair_cosine is defined before it and
// keeps the contraction it has in every other file), so neither the cut seg_start + (p + 0.5) * hop_ms / 1000.0 nor the tests
// cut - last >= min_speech_s can become a fused operation: the times are the host's f64 values.
//
// Nothing is read from first_row or first_piece and used as an address before the whole promise about both tables has been checked.
#include <hip/hip_runtime.h>

#include "sd_common.h"
#include "sd_hip_scd.h"
#include "scd/sd_scd_check.h"

#pragma clang fp contract(off)

static_assert(SD_SCD_S_LDS_ROWS == SD_SCD_LDS_ROWS, "the header names the LDS limit of the kernel");

namespace {

constexpr int SC_THREADS = SD_SCD_THREADS, SC_WAVES = SC_THREADS / 64;

// The sum of v over the 256 threads, the same bits in every thread: a butterfly inside each wave (a + b is b + a, so every lane of a
// wave holds one value), then the waves in order.  s_w: SC_WAVES doubles of LDS.  Called by every thread; two barriers, the first of
// which lets the readers of the last call finish.
__device__ __forceinline__ double sc_sum(double v, double* s_w) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double sum = s_w[0];
  for (int w = 1; w < SC_WAVES; ++w) sum += s_w[w];
  return sum;
}

// The exclusive prefix sum of v over the 256 threads, and the sum of all of them in *total.  s_w: SC_WAVES words of LDS.  Barriers
// as in sc_sum.
__device__ __forceinline__ int sc_scan_sum(const int v, int* s_w, int* total) {
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
  for (int w = 0; w < SC_WAVES; ++w) {
    const int t = s_w[w];
    before += w < wave ? t : 0;
    sum += t;
  }
  *total = sum;
  return before + inc - v;
}

// The inclusive maximum of v over the threads 0 .. this one, and the maximum over all of them in *all.  Barriers as in sc_sum.
__device__ __forceinline__ int sc_scan_max(const int v, int* s_w, int* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc, d);
    if (lane >= d && up > inc) inc = up;
  }
  __syncthreads();
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int top = s_w[0];
  for (int w = 0; w < SC_WAVES; ++w) {
    const int t = s_w[w];
    if (w < wave && t > inc) inc = t;
    if (t > top) top = t;
  }
  *all = top;
  return inc;
}

// rule 6, the operations in the host's order: (p + 0.5) * hop_ms, then / 1000.0, then seg_start + that
__device__ __forceinline__ double sc_cut(const double seg_start, const int p, const double hop_ms) {
  const double a = (double)p + 0.5;
  const double b = a * hop_ms;
  const double c = b / 1000.0;
  return seg_start + c;
}

__global__ __launch_bounds__(SC_THREADS) void scd_split_kernel(const float* __restrict__ rows, const int ld, const int dim, const int n_rows,
                                                               const int* __restrict__ first_row, const int n_segs,
                                                               const double* __restrict__ seg_start, const double* __restrict__ seg_end,
                                                               const double hop_ms, const double thr, const double min_speech_s,
                                                               const float eps, const int* __restrict__ first_piece, const int piece_cap,
                                                               int* __restrict__ n_peaks, int* __restrict__ n_pieces,
                                                               double* __restrict__ piece_start, double* __restrict__ piece_end,
                                                               float* __restrict__ sims, unsigned char* __restrict__ peak_mask,
                                                               int* __restrict__ bad, unsigned char* ws) {
  __shared__ double s_cut[SD_SCD_S_LDS_CUTS];
  __shared__ float s_dist[SD_SCD_S_LDS_ROWS];
  __shared__ int s_next[SD_SCD_S_LDS_CUTS];
  __shared__ double s_wd[SC_WAVES];
  __shared__ int s_wi[SC_WAVES];
  __shared__ int s_bad;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float nan32 = __uint_as_float(0x7fc00000u);
  if (tid == 0) s_bad = 0;
  __syncthreads();

  // the promise about first_row and first_piece, all of it: the slices of the segments are disjoint only under it
  for (int i = tid; i <= n_segs; i += SC_THREADS) {
    const int fr = first_row[i], fp = first_piece[i];
    bool broken = fr < 0 || fr > n_rows || fp < 0 || fp > piece_cap || (i == 0 && (fr != 0 || fp != 0)) ||
                  (i == n_segs && (fr != n_rows || fp != piece_cap));
    if (i < n_segs) broken |= first_row[i + 1] < fr || first_piece[i + 1] < fp;
    if (broken) s_bad = 1;                               // every thread that finds it stores the same 1
  }
  __syncthreads();
  if (s_bad != 0) {                                      // no segment has a slice of its own: every workgroup fills its share of the rows
    const long long from = (long long)n_rows * g / n_segs, to = (long long)n_rows * (g + 1) / n_segs;
    for (long long p = from + tid; p < to; p += SC_THREADS) {
      if (sims) sims[p] = nan32;
      if (peak_mask) peak_mask[p] = 0;
    }
    if (tid == 0) bad[g] = SD_SCD_BAD_PROMISE, n_peaks[g] = 0, n_pieces[g] = 0;
    return;
  }
  const int r0 = first_row[g], n = first_row[g + 1] - r0;                  // 0 <= r0, r0 + n <= n_rows, disjoint from every other's
  const int q0 = first_piece[g], cap = first_piece[g + 1] - q0;            // 0 <= q0, q0 + cap <= piece_cap, likewise
  if (peak_mask) for (int i = tid; i < n; i += SC_THREADS) peak_mask[r0 + i] = 0;
  if (cap < sd_scd_piece_capacity(n)) {
    if (sims) for (int i = tid; i < n; i += SC_THREADS) sims[r0 + i] = nan32;
    if (tid == 0) bad[g] = SD_SCD_BAD_CAPACITY, n_peaks[g] = 0, n_pieces[g] = 0;
    return;
  }
  const double t0 = seg_start[g], t1 = seg_end[g];
  const int m = n - 1;

  // ---- (a) the cosines of the pairs (for `sims` alone when the segment is too short to split)
  const bool in_lds = n <= SD_SCD_S_LDS_ROWS;
  double* const cut = in_lds ? s_cut : reinterpret_cast<double*>(ws) + r0;
  float* const dist = in_lds ? s_dist : reinterpret_cast<float*>(ws + sd_scd_ws_dist_offset(n_rows)) + r0;
  int* const next = in_lds ? s_next : reinterpret_cast<int*>(ws + sd_scd_ws_chain_offset(n_rows)) + r0;
  if (n >= 3 || sims) {
    const float* const x = rows + (long long)r0 * ld;
    for (int i = wave; i < m; i += SC_WAVES) {
      const float s = sd_wave_pair_cosine(x + (long long)i * ld, x + (long long)(i + 1) * ld, dim, eps, lane);
      if (lane == 0) {
        if (n >= 3) dist[i] = 1.f - s;
        if (sims) sims[r0 + i] = s;
      }
    }
    if (sims && n > 0 && tid == 0) sims[r0 + m] = nan32;
  }
  if (n < 3) {                                           // rule 1 (cap >= 1)
    if (tid == 0) bad[g] = 0, n_peaks[g] = 0, n_pieces[g] = 1, piece_start[q0] = t0, piece_end[q0] = t1;
    return;
  }
  __syncthreads();                                       // the distances, and the zeros of the mask, are in place

  // ---- (b) mean and population std in f64
  double acc = 0.0;
  for (int i = tid; i < m; i += SC_THREADS) acc += (double)dist[i];
  const double mean = sc_sum(acc, s_wd) / (double)m;
  acc = 0.0;
  for (int i = tid; i < m; i += SC_THREADS) {
    const double t = (double)dist[i] - mean;
    acc += t * t;
  }
  const double sd = sqrt(sc_sum(acc, s_wd) / (double)m);
  const bool use_z = sd > 1e-6;                          // false for a NaN

  // ---- (c) peaks.  At most (m - 1) / 2 of them: two peaks have a lower value between them, and neither end is one.
  int last_start = -1, K = 0;                            // last_start: the start of the run that the element before this step is in
  for (int base = 0; base < m; base += SC_THREADS) {     // uniform: every thread reaches the scans
    const int i = base + tid;
    const bool in = i < m;
    const float v = in ? dist[i] : 0.f;
    const bool has_next = in && i + 1 < m;
    const float vn = has_next ? dist[i + 1] : 0.f;
    const bool starts = in && (i == 0 || !(dist[i - 1] == v));
    int top;
    int l = sc_scan_max(starts ? i : -1, s_wi, &top);
    l = l > last_start ? l : last_start;                 // 0 <= l <= i for i < m: element 0 starts a run
    last_start = top > last_start ? top : last_start;
    const bool peak = has_next && vn < v && l >= 1 && dist[l - 1] < v;     // the run [l, i]: a fall after it, a rise before it
    const int p = (l + i) >> 1;
    const double z = use_z ? ((double)v - mean) / sd : (double)v;         // z[p]: the run's value is one value
    const bool keep = peak && z >= thr;
    int total;
    const int rank = sc_scan_sum(keep ? 1 : 0, s_wi, &total);
    if (keep) {
      cut[K + rank] = sc_cut(t0, p, hop_ms);             // K + rank < (m - 1) / 2 + 1 <= n / 2
      if (peak_mask) peak_mask[r0 + p] = 1;              // cleared above, and barriers since
    }
    K += total;
  }
  __syncthreads();
  if (K == 0) {                                          // rule 5
    if (tid == 0) bad[g] = 0, n_peaks[g] = 0, n_pieces[g] = 1, piece_start[q0] = t0, piece_end[q0] = t1;
    return;
  }

  // ---- (d) next(j): the first later cut that differs from cut j (rule 6) and lies min_speech_s or more after it; K when there is none.
  // cut[] does not decrease and x - c rounds monotonically in x, so the test is false up to some index and true from it on.
  for (int j = tid; j < K; j += SC_THREADS) {
    const double c = cut[j];
    int lo = j + 1, hi = K;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      const double x = cut[mid];
      if (x != c && x - c >= min_speech_s) hi = mid;
      else lo = mid + 1;
    }
    next[j] = lo;                                        // j < lo <= K
  }
  __syncthreads();
  if (tid == 0) {
    int lo = 0, hi = K;                                  // the first cut that the start of the segment accepts
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cut[mid] - t0 >= min_speech_s) hi = mid;
      else lo = mid + 1;
    }
    double last = t0;
    int pieces = 0;
    for (int j = lo; j < K; j = next[j]) {               // strictly increasing j: at most K links, each one piece; K + 1 <= cap
      const double c = cut[j];
      piece_start[q0 + pieces] = last, piece_end[q0 + pieces] = c;
      ++pieces;
      last = c;
    }
    if (t1 - last >= min_speech_s) {
      piece_start[q0 + pieces] = last, piece_end[q0 + pieces] = t1;
      ++pieces;
    }
    bad[g] = 0, n_peaks[g] = K, n_pieces[g] = pieces;
  }
}

}  // namespace

extern "C" int sd_scd_abi_version(void) { return SD_SCD_ABI_VERSION; }

extern "C" size_t sd_scd_split_workspace_bytes(int n_rows, int n_segs) { return sd_scd_workspace_bytes(n_rows, n_segs); }

extern "C" int sd_scd_split_grouped_f32(const float* rows, int ld, int dim, int n_rows, const int* first_row, int n_segs,
                                        const double* seg_start, const double* seg_end, double hop_ms, double thr, double min_speech_s,
                                        float eps, const int* first_piece, int piece_cap, int* n_peaks, int* n_pieces, double* piece_start,
                                        double* piece_end, float* sims, unsigned char* peak_mask, int* bad, void* ws, size_t ws_bytes,
                                        sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SdScdCall c = {};
  c.ld = ld, c.dim = dim, c.n_rows = n_rows, c.n_segs = n_segs, c.piece_cap = piece_cap;
  c.hop_ms = hop_ms, c.thr = thr, c.min_speech_s = min_speech_s, c.eps = eps;
  c.table_null = !(first_row && seg_start && seg_end && first_piece && n_peaks && n_pieces && bad);
  c.rows_null = !(rows && ws);
  c.pieces_null = !(piece_start && piece_end);
  c.ws_misaligned = !sd_aligned16(ws);
  c.ws_bytes = ws_bytes;
  char why[SD_SCD_WHY];
  if (const int e = sd_scd_check(c, why)) return sd_set_error(e, "%s", why);
  hipLaunchKernelGGL(scd_split_kernel, dim3((unsigned)n_segs), dim3(SC_THREADS), 0, stream, rows, ld, dim, n_rows, first_row, n_segs, seg_start,
                     seg_end, hop_ms, thr, min_speech_s, eps, first_piece, piece_cap, n_peaks, n_pieces, piece_start, piece_end, sims, peak_mask,
                     bad, static_cast<unsigned char*>(ws));
  SD_CHECK_LAUNCH("scd_split_kernel");
  return SD_OK;
}
