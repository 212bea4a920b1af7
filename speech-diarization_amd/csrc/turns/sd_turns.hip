// Speaker turns for MANY recordings at once (include/sd_hip_turns.h): the window labels of a recording to its relabelled labels and
// its (region, first frame, end frame, label) runs.  DESIGN.md section 26 has the argument.
//
// turns_kernel          a workgroup owns a recording of n windows; every step runs on all 256 threads.
//   (a) checks          the promise about first_window and first_region, all of it (every workgroup: the slices are disjoint only
//                       under it); then the recording's own labels, its slice of region_first_window, its frame counts, and per window
//                       the margin between neighbouring centres (rule 4).  A flagged recording stops here, nothing of it written
//   (b) relabel         table A: the first window of every label, by an integer minimum (only a window whose predecessor carries
//                       another label can be the first of its label); 256 windows at a time, a prefix sum over "this window is the
//                       first of its label" numbers the labels into table B; new_labels = B[label]
//   (c) first frames    table A: f_j, the first frame that is nearer to window j than to window j - 1 (0 for a region's first
//                       window), by binary search; table B: the window's region
//   (d) runs            256 windows at a time: window j owns frames iff f_j < f_{j + 1} (n_frames after the region's last window);
//                       "the last owner before this window" by a block scan with the operator max; an owner is the head of a run
//                       iff that owner lies in another region or carries another new label; a prefix sum ranks the heads
//   (e) ends            run k ends where run k + 1 begins when both lie in one region, at n_frames otherwise
// The two tables live in LDS up to SD_TURNS_LDS_WINDOWS windows and in the recording's slice of `ws` above that.
//
// Contraction: the whole file is compiled with `fp contract(off)`, so the frame time region_start + (i + 0.5) * frame_s cannot become a
// fused operation: the distances are the host's f64 values.
//
// Nothing is read from a table and used as an address before the promise that bounds it has been checked.
#include <hip/hip_runtime.h>

#include "sd_common.h"
#include "sd_hip_turns.h"
#include "turns/sd_turns_check.h"

#pragma clang fp contract(off)

static_assert(SD_TURNS_T_LDS_WINDOWS == SD_TURNS_LDS_WINDOWS, "the header names the LDS limit of the kernel");

namespace {

constexpr int TN_THREADS = SD_TURNS_THREADS, TN_WAVES = TN_THREADS / 64;

// The exclusive prefix sum of v over the 256 threads, and the sum of all of them in *total.  s_w: TN_WAVES words of LDS.  Called by
// every thread; two barriers, the first of which lets the readers of the last call finish.
__device__ __forceinline__ int tn_scan_sum(const int v, int* s_w, int* total) {
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
  for (int w = 0; w < TN_WAVES; ++w) {
    const int t = s_w[w];
    before += w < wave ? t : 0;
    sum += t;
  }
  *total = sum;
  return before + inc - v;
}

// The maximum of v (>= -1) over the threads BEFORE this one, -1 for thread 0, and the maximum over all of them in *all.  Barriers as
// in tn_scan_sum.
__device__ __forceinline__ int tn_scan_max_before(const int v, int* s_w, int* all) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc, d);
    if (lane >= d && up > inc) inc = up;
  }
  __syncthreads();
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  const int left = __shfl_up(inc, 1);
  int before = lane == 0 ? -1 : left, top = -1;
  for (int w = 0; w < TN_WAVES; ++w) {
    const int t = s_w[w];
    if (w < wave && t > before) before = t;
    if (t > top) top = t;
  }
  *all = top;
  return before;
}

// rule 2, the operations in the host's order: (i + 0.5) * frame_s, then region_start + that
__device__ __forceinline__ double tn_time(const double region_start, const int i, const double frame_s) {
  const double a = (double)i + 0.5;
  const double b = a * frame_s;
  return region_start + b;
}

// The region (counted inside the recording) of window w: the last q < nr with rfw[q] <= w.  rfw: the recording's slice, nr + 1
// entries that do not decrease, rfw[0] <= w < rfw[nr]; every index read lies in [0, nr).
__device__ __forceinline__ int tn_region_of(const int* rfw, const int nr, const int w) {
  int lo = 0, hi = nr - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rfw[mid] <= w) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(TN_THREADS) void turns_kernel(const int* __restrict__ first_window, const int* __restrict__ first_region,
                                                           const int n_recordings, const int* __restrict__ region_first_window,
                                                           const int n_regions, const double* __restrict__ centre, const int n_windows,
                                                           const double* __restrict__ region_start, const int* __restrict__ n_frames,
                                                           const double frame_s, const int* __restrict__ labels, int* new_labels,
                                                           int* __restrict__ n_runs, int* run_region, int* run_first,
                                                           int* __restrict__ run_end, int* __restrict__ run_label, int* __restrict__ bad,
                                                           unsigned char* ws) {
  __shared__ int s_a[SD_TURNS_T_LDS_WINDOWS];
  __shared__ int s_b[SD_TURNS_T_LDS_WINDOWS];
  __shared__ int s_wi[TN_WAVES];
  __shared__ int s_tables, s_flag;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_tables = 0, s_flag = 0;
  __syncthreads();

  // ---- (a) the promise about first_window and first_region, all of it: the slices of the recordings are disjoint only under it
  for (int i = tid; i <= n_recordings; i += TN_THREADS) {
    const int fw = first_window[i], fr = first_region[i];
    bool broken = fw < 0 || fw > n_windows || fr < 0 || fr > n_regions || (i == 0 && (fw != 0 || fr != 0)) ||
                  (i == n_recordings && (fw != n_windows || fr != n_regions));
    if (i < n_recordings) broken |= first_window[i + 1] < fw || first_region[i + 1] < fr;
    if (broken) s_tables = 1;                            // every thread that finds it stores the same 1
  }
  __syncthreads();
  if (s_tables != 0) {
    if (tid == 0) bad[g] = SD_TURNS_BAD_PROMISE, n_runs[g] = 0;
    return;
  }
  const int w0 = first_window[g], n = first_window[g + 1] - w0;            // 0 <= w0, w0 + n <= n_windows, disjoint from every other's
  const int r0 = first_region[g], nr = first_region[g + 1] - r0;           // 0 <= r0, r0 + nr <= n_regions
  const int* const rfw = region_first_window + r0;                         // nr + 1 entries: region_first_window has n_regions + 1

  // the recording's labels, its slice of region_first_window and its frame counts
  for (int i = tid; i < n; i += TN_THREADS)
    if (labels[w0 + i] >= n) atomicOr(&s_flag, SD_TURNS_BAD_LABEL);
  for (int q = tid; q <= nr; q += TN_THREADS) {
    const int a = rfw[q];
    bool broken = a < w0 || a > w0 + n || (q == 0 && a != w0) || (q == nr && a != w0 + n);
    if (q < nr) broken |= rfw[q + 1] < a || n_frames[r0 + q] < 1;
    if (broken) atomicOr(&s_flag, SD_TURNS_BAD_PROMISE);
  }
  __syncthreads();
  const bool regions_ok = (s_flag & SD_TURNS_BAD_PROMISE) == 0;
  __syncthreads();                                       // every thread has read the flag before the loop below may set it
  // Per window, the margin of rule 4.  The region's windows [a, b] lie inside [w0, w0 + n) now, so centre[] is read inside the slice.
  if (regions_ok) {
    for (int i = tid; i < n; i += TN_THREADS) {
      const int w = w0 + i, q = tn_region_of(rfw, nr, w);
      const int a = rfw[q], b = rfw[q + 1] - 1;          // a <= w <= b
      const double s = region_start[r0 + q];
      const double t_0 = tn_time(s, 0, frame_s), t_last = tn_time(s, n_frames[r0 + q] - 1, frame_s);
      const double c_a = centre[a], c_b = centre[b];
      const double d0 = fabs(t_0 - c_a), d1 = fabs(t_0 - c_b), d2 = fabs(t_last - c_a), d3 = fabs(t_last - c_b);
      bool ok = d0 <= __DBL_MAX__ && d1 <= __DBL_MAX__ && d2 <= __DBL_MAX__ && d3 <= __DBL_MAX__;      // false for an infinity and for a NaN
      double E = d0;
      E = d1 > E ? d1 : E;
      E = d2 > E ? d2 : E;
      E = d3 > E ? d3 : E;
      if (w > a) ok = ok && centre[w] - centre[w - 1] >= E * 0x1p-40;
      if (!ok) atomicOr(&s_flag, SD_TURNS_BAD_PROMISE);
    }
  }
  __syncthreads();
  if (s_flag != 0) {                                     // nothing of the recording is written but its two words
    if (tid == 0) bad[g] = s_flag, n_runs[g] = 0;
    return;
  }

  const bool in_lds = n <= SD_TURNS_T_LDS_WINDOWS;      // n above it: n_windows is too, and the entry has checked `ws` for 8 n_windows bytes
  int* const ta = in_lds ? s_a : reinterpret_cast<int*>(ws) + w0;
  int* const tb = in_lds ? s_b : reinterpret_cast<int*>(ws + sd_turns_ws_b_offset(n_windows)) + w0;

  // ---- (b) relabel.  Every label is below n (checked), so it indexes the tables.
  for (int i = tid; i < n; i += TN_THREADS) ta[i] = n;
  __syncthreads();
  for (int i = tid; i < n; i += TN_THREADS) {
    const int lab = labels[w0 + i];
    if (lab >= 0 && (i == 0 || labels[w0 + i - 1] != lab)) atomicMin(&ta[lab], i);
  }
  __syncthreads();
  int numbered = 0;
  for (int base = 0; base < n; base += TN_THREADS) {     // uniform: every thread reaches the scan
    const int i = base + tid;
    const int lab = i < n ? labels[w0 + i] : -1;
    const bool first = lab >= 0 && ta[lab] == i;
    int total;
    const int rank = tn_scan_sum(first ? 1 : 0, s_wi, &total);
    if (first) tb[lab] = numbered + rank;
    numbered += total;
  }
  __syncthreads();
  for (int i = tid; i < n; i += TN_THREADS) {
    const int lab = labels[w0 + i];
    new_labels[w0 + i] = lab < 0 ? -1 : tb[lab];
  }
  __syncthreads();                                       // the tables are free, and the new labels are in place for every thread

  // ---- (c) f_j: "nearer to window j than to window j - 1" is false up to some frame and true from it on (rule 4)
  for (int i = tid; i < n; i += TN_THREADS) {
    const int w = w0 + i, q = tn_region_of(rfw, nr, w);
    int f = 0;
    if (w > rfw[q]) {
      const double c = centre[w], c_before = centre[w - 1], s = region_start[r0 + q];
      int lo = 0, hi = n_frames[r0 + q];
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const double t = tn_time(s, mid, frame_s);
        if (fabs(t - c) < fabs(t - c_before)) hi = mid;
        else lo = mid + 1;
      }
      f = lo;                                            // n_frames when no frame is nearer to it
    }
    ta[i] = f, tb[i] = q;
  }
  __syncthreads();

  // ---- (d) runs.  A head is an owner, so there are at most n of them: the slots w0 + K + rank stay inside the recording's slice.
  int last_owner = -1, K = 0;
  for (int base = 0; base < n; base += TN_THREADS) {
    const int i = base + tid;
    const bool in = i < n;
    const int q = in ? tb[i] : -1, f = in ? ta[i] : 0;
    int f_next = 0;
    if (in) f_next = i + 1 < n && tb[i + 1] == q ? ta[i + 1] : n_frames[r0 + q];
    const bool owns = in && f < f_next;
    int top;
    int p = tn_scan_max_before(owns ? i : -1, s_wi, &top);
    p = p > last_owner ? p : last_owner;                 // the last owner before window i, -1 when there is none
    last_owner = top > last_owner ? top : last_owner;
    const int lab = in ? new_labels[w0 + i] : 0;
    const bool head = owns && (p < 0 || tb[p] != q || new_labels[w0 + p] != lab);
    int total;
    const int rank = tn_scan_sum(head ? 1 : 0, s_wi, &total);
    if (head) {
      const int k = w0 + K + rank;
      run_region[k] = q, run_first[k] = f, run_label[k] = lab;
    }
    K += total;
  }
  __syncthreads();

  // ---- (e) ends
  for (int k = tid; k < K; k += TN_THREADS) {
    const int q = run_region[w0 + k];
    run_end[w0 + k] = k + 1 < K && run_region[w0 + k + 1] == q ? run_first[w0 + k + 1] : n_frames[r0 + q];
  }
  if (tid == 0) bad[g] = 0, n_runs[g] = K;
}

}  // namespace

extern "C" int sd_turns_abi_version(void) { return SD_TURNS_ABI_VERSION; }

extern "C" size_t sd_turns_workspace_bytes(int n_windows, int n_recordings) { return sd_turns_ws_bytes(n_windows, n_recordings); }

extern "C" int sd_turns_grouped(const int* first_window, const int* first_region, int n_recordings, const int* region_first_window,
                                int n_regions, const double* centre, int n_windows, const double* region_start, const int* n_frames,
                                double frame_s, const int* labels, int* new_labels, int* n_runs, int* run_region, int* run_first,
                                int* run_end, int* run_label, int* bad, void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SdTurnsCall c = {};
  c.n_recordings = n_recordings, c.n_regions = n_regions, c.n_windows = n_windows, c.frame_s = frame_s;
  c.table_null = !(first_window && first_region && region_first_window && n_runs && bad);
  c.region_null = !(region_start && n_frames);
  c.window_null = !(centre && labels && new_labels && run_region && run_first && run_end && run_label);
  c.ws_null = !ws;
  c.ws_misaligned = !sd_aligned16(ws);
  c.ws_bytes = ws_bytes;
  char why[SD_TURNS_WHY];
  if (const int e = sd_turns_check(c, why)) return sd_set_error(e, "%s", why);
  const bool uses_ws = sd_turns_need(c) != 0;
  hipLaunchKernelGGL(turns_kernel, dim3((unsigned)n_recordings), dim3(TN_THREADS), 0, stream, first_window, first_region, n_recordings,
                     region_first_window, n_regions, centre, n_windows, region_start, n_frames, frame_s, labels, new_labels, n_runs, run_region,
                     run_first, run_end, run_label, bad, static_cast<unsigned char*>(ws));
  SD_CHECK_LAUNCH(uses_ws ? "turns_kernel/ws" : "turns_kernel/lds");
  return SD_OK;
}
