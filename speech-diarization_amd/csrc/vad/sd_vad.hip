// Voice activity for MANY recordings at once (include/sd_hip_vad.h): the frame scores of the stand-in scorer, and frame probabilities
// to speech runs.  DESIGN.md section 24 has the argument.
//
// vad_energy_kernel     a workgroup owns 64 consecutive frames of `probs`.  It finds the recording of its first frame by a bounded
//                       search, checks what it read, stages the samples of its frames of that recording once, and moves on to the next
//                       recording while frames are left.  A wave sums one frame in f64, lane l the samples l, l + 64, ...
// vad_segments_kernel   a workgroup owns a recording.
//   (a) runs            1 024 frames at a time: the event of each frame (start 1, stop 2, none 0), a block scan with the operator "last
//                       non-zero", the speech bit of the frame before, and the flags "a run starts here" / "a run ended here"; a prefix
//                       sum of the flags ranks them into the run list (start[], end[]).
//   (b) opening         keep the runs of at least open_len frames                        (filter)
//   (c) closing         join runs less than close_len apart                              (join)
//                       clip to [c, n - (close_len - 1 - c)) and drop what is empty      (filter); the mask is written from this list
//   (d) run rules       keep the runs of at least min_run frames                         (filter)
//                       join runs at most max_gap apart                                  (join)
//                       Filter and join work on the run list in place, 1 024 runs at a time: every run of a step is read, a prefix sum
//                       ranks what stays, and a run is stored at its rank, which is at most its own position.
//
// Nothing is read from first_sample, n_samples, first_frame or first_seg and used as an address before it is compared with its range.
#include <hip/hip_runtime.h>

#include "sd_common.h"
#include "sd_hip_vad.h"
#include "vad/sd_vad_check.h"

static_assert(SD_VAD_S_LDS_FRAMES == SD_VAD_LDS_FRAMES, "the header names the LDS limit of the segments kernel");

namespace {

// ================================================================================================ energy

// The `bad` word of recording g (0: every range below holds).  Pure in the tables: every workgroup that asks gets the same answer.
__device__ __forceinline__ int ve_check(const int g, const long long n_signal, const long long* __restrict__ first_sample,
                                        const int* __restrict__ n_samples, const int n_groups, const int win, const int hop,
                                        const int* __restrict__ first_frame, const int n_frames) {
  const int ns = n_samples[g], lo = first_frame[g], hi = first_frame[g + 1];
  const long long fs = first_sample[g];
  int bits = 0;
  if (ns < win) bits |= SD_VAD_SHORT;
  if (ns < 0 || fs < 0 || fs > n_signal - (long long)ns) bits |= SD_VAD_BAD_RANGE;
  const long long count = ns >= win ? 1 + (long long)(ns - win) / hop : 0;
  if (lo < 0 || hi > n_frames || (long long)hi - (long long)lo != count || (g == 0 && lo != 0) || (g == n_groups - 1 && hi != n_frames))
    bits |= SD_VAD_BAD_FRAMES;
  return bits;
}

// lane l of a wave: the squares of x[l], x[l + 64], ... added in f64 in that order; the same code for staged and for global samples
template <typename P>
__device__ __forceinline__ double ve_lane_sum(const P x, const int win, const int lane) {
  double acc = 0.0;
  for (int i = lane; i < win; i += 64) {
    const double v = (double)x[i];
    acc += v * v;                                        // exact product: 48 bits of an f64's 53
  }
  return acc;
}

__global__ __launch_bounds__(SD_VAD_E_THREADS) void vad_energy_kernel(const float* __restrict__ signal, const long long n_signal,
                                                                      const long long* __restrict__ first_sample,
                                                                      const int* __restrict__ n_samples, const int n_groups, const int win,
                                                                      const int hop, const float threshold_db, const float slope,
                                                                      const int* __restrict__ first_frame, const int n_frames,
                                                                      float* __restrict__ probs, int* __restrict__ bad) {
  __shared__ float s_x[SD_VAD_E_STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (long long g = (long long)blockIdx.x * SD_VAD_E_THREADS + tid; g < n_groups; g += (long long)gridDim.x * SD_VAD_E_THREADS)
    bad[g] = ve_check((int)g, n_signal, first_sample, n_samples, n_groups, win, hop, first_frame, n_frames);

  const long long t0l = (long long)blockIdx.x * SD_VAD_E_TILE;
  if (t0l >= n_frames) return;                           // the one workgroup of a launch without frames
  const int t0 = (int)t0l, t1 = n_frames - t0 < SD_VAD_E_TILE ? n_frames : t0 + SD_VAD_E_TILE;
  int f = t0;                                            // workgroup-uniform, as everything that steers the loop
  while (f < t1) {
    const int g = sd_span_of(first_frame, n_groups, f);  // in [0, n_groups) for any table
    const int lo = first_frame[g], hi = first_frame[g + 1];
    const bool ok = lo <= f && f < hi && ve_check(g, n_signal, first_sample, n_samples, n_groups, win, hop, first_frame, n_frames) == 0;
    if (!ok) {                                           // a frame of a bad recording, or of none
      if (tid == 0) probs[f] = __uint_as_float(0x7fc00000u);
      ++f;
      continue;
    }
    const int end = hi < t1 ? hi : t1, count = end - f;  // 1 <= count <= 64
    // checked: the samples [fs, fs + ns) lie inside the signal and hold the frames lo .. hi - 1 of the recording
    const long long base = first_sample[g] + (long long)(f - lo) * hop;
    const long long span = (long long)(count - 1) * hop + win;
    const bool staged = span <= SD_VAD_E_STAGE;
    __syncthreads();                                     // the readers of the last staging are done
    if (staged)
      for (int i = tid; i < (int)span; i += SD_VAD_E_THREADS) s_x[i] = signal[base + i];
    __syncthreads();
    for (int j = wave; j < count; j += SD_VAD_E_THREADS / 64) {
      double acc = staged ? ve_lane_sum(s_x + (long long)j * hop, win, lane) : ve_lane_sum(signal + base + (long long)j * hop, win, lane);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);      // one tree for every lane: a + b is b + a
      if (lane == 0) {
        double m = acc / (double)win;
        m = m < 1e-12 ? 1e-12 : m;                       // a NaN stays
        const double db = 20.0 * log10(sqrt(m));
        const double z = (double)slope * (db - (double)threshold_db);
        probs[f + j] = (float)(1.0 / (1.0 + exp(-z)));
      }
    }
    f = end;
  }
}

// ================================================================================================ segments

constexpr int VS_THREADS = SD_VAD_S_THREADS, VS_WAVES = VS_THREADS / 64;

// The exclusive prefix sum of v over the 1 024 threads, and the sum of all of them in *total.  s_w: 16 words of LDS.  Called by every
// thread of the workgroup; two barriers, the first of which lets the readers of the last call finish.
__device__ __forceinline__ int vs_scan(const int v, int* s_w, int* total) {
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
  for (int w = 0; w < VS_WAVES; ++w) {
    const int t = s_w[w];
    before += w < wave ? t : 0;
    sum += t;
  }
  *total = sum;
  return before + inc - v;
}

// Filter: every run clipped to [lo, hi); it stays when it is not empty and has at least min_len frames.  -> the runs that stay.
__device__ int vs_filter(int* rs, int* re, const int K, const int min_len, const int lo, const int hi, int* s_w) {
  int out = 0;
  for (int base = 0; base < K; base += VS_THREADS) {     // uniform: every thread reaches the scan
    const int k = base + threadIdx.x;
    int s = 0, e = 0;
    bool keep = false;
    if (k < K) {
      s = rs[k], e = re[k];
      s = s > lo ? s : lo, e = e < hi ? e : hi;
      keep = e > s && e - s >= min_len;
    }
    int total;
    const int before = vs_scan(keep ? 1 : 0, s_w, &total);     // its barriers stand between the reads above and the stores below
    if (keep) rs[out + before] = s, re[out + before] = e;      // at most position k; later steps read from base + 1024 on
    out += total;
  }
  __syncthreads();
  return out;
}

// Join: consecutive runs at most max_gap frames apart become one.  -> the runs that are left.  s_a, s_b: 1 024 words of LDS each.
__device__ int vs_join(int* rs, int* re, const int K, const int max_gap, int* s_w, int* s_a, int* s_b) {
  int out = 0, carry_e = 0;                              // carry_e: the end of run base - 1 as it was before this call
  for (int base = 0; base < K; base += VS_THREADS) {
    const int tid = threadIdx.x, k = base + tid;
    int s = 0, e = 0;
    if (k < K) s = rs[k], e = re[k];
    s_a[tid] = s, s_b[tid] = e;
    int s_after = 0;
    if (tid == VS_THREADS - 1 && k + 1 < K) s_after = rs[k + 1];           // position base + 1024: not stored to yet
    __syncthreads();
    const int e_before = tid ? s_b[tid - 1] : carry_e;
    if (tid < VS_THREADS - 1) s_after = s_a[tid + 1];
    carry_e = s_b[VS_THREADS - 1];
    const bool opens = k < K && (k == 0 || s - e_before > max_gap);
    const bool closes = k < K && (k == K - 1 || s_after - e > max_gap);
    int total;
    const int before = vs_scan(opens ? 1 : 0, s_w, &total);               // two barriers: s_a and s_b are free again after them
    const int r = out + before + (opens ? 1 : 0) - 1;                     // the joined run this one belongs to: 0 <= r <= k for k < K
    if (opens) rs[r] = s;
    if (closes) re[r] = e;
    out += total;
  }
  __syncthreads();
  return out;
}

__global__ __launch_bounds__(VS_THREADS) void vad_segments_kernel(const float* __restrict__ probs, const int* __restrict__ first_frame,
                                                                  const int n_groups, const int n_frames, const float on, const float off,
                                                                  const int open_len, const int close_len, const int min_run,
                                                                  const int max_gap, const int* __restrict__ first_seg, const int seg_cap,
                                                                  int* __restrict__ n_segs, int* __restrict__ seg_start,
                                                                  int* __restrict__ seg_end, unsigned char* __restrict__ mask,
                                                                  int* __restrict__ bad, int* ws) {
  extern __shared__ __attribute__((aligned(16))) int s_runs[];             // 2 x SD_VAD_S_LDS_RUNS
  __shared__ int s_a[VS_THREADS], s_b[VS_THREADS];
  __shared__ int s_w[VS_WAVES];
  __shared__ int s_bad;
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_bad = 0;
  __syncthreads();

  // the promise about first_frame and first_seg, all of it: the slices of the recordings are disjoint only under it
  for (int i = tid; i <= n_groups; i += VS_THREADS) {
    const int ff = first_frame[i], fs = first_seg[i];
    bool broken = ff < 0 || ff > n_frames || fs < 0 || fs > seg_cap || (i == 0 && (ff != 0 || fs != 0)) ||
                  (i == n_groups && (ff != n_frames || fs != seg_cap));
    if (i < n_groups) broken |= first_frame[i + 1] < ff || first_seg[i + 1] < fs;
    if (broken) s_bad = 1;                                                 // every thread that finds it stores the same 1
  }
  __syncthreads();
  if (s_bad != 0) {                                      // no recording has a slice of its own: every workgroup clears its share of the mask
    if (mask) {
      const long long from = (long long)n_frames * g / n_groups, to = (long long)n_frames * (g + 1) / n_groups;
      for (long long p = from + tid; p < to; p += VS_THREADS) mask[p] = 0;
    }
    if (tid == 0) bad[g] = SD_VAD_BAD_PROMISE, n_segs[g] = 0;
    return;
  }
  const int f0 = first_frame[g], n = first_frame[g + 1] - f0;              // 0 <= f0, f0 + n <= n_frames, disjoint from every other's
  const int q0 = first_seg[g], cap = first_seg[g + 1] - q0;                // 0 <= q0, q0 + cap <= seg_cap, likewise
  const float* const p = probs + f0;
  unsigned char* const m = mask ? mask + f0 : nullptr;
  if (m) for (int i = tid; i < n; i += VS_THREADS) m[i] = 0;
  if (cap < (n + 1) / 2) {
    if (tid == 0) bad[g] = SD_VAD_BAD_CAPACITY, n_segs[g] = 0;
    return;
  }
  const bool in_lds = n <= SD_VAD_S_LDS_FRAMES;                            // (n + 1) / 2 <= SD_VAD_S_LDS_RUNS
  int* const rs = in_lds ? s_runs : ws + q0;
  int* const re = in_lds ? s_runs + SD_VAD_S_LDS_RUNS : ws + seg_cap + q0;

  // ---- (a) hysteresis and the run list.  A mask of n frames has at most (n + 1) / 2 runs, so no rank reaches the capacity.
  int carry = 0, n_starts = 0, n_ends = 0;                                 // carry: the last event before this step (0: none yet)
  for (int base = 0; base < n; base += VS_THREADS) {
    const int i = base + tid;
    int ev = 0;
    if (i < n) {
      const float v = p[i];
      ev = v >= on ? 1 : (v < off ? 2 : 0);                                // on > off: never both; a NaN is neither
    }
    int inc = ev;
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(inc, d);
      if (lane >= d && inc == 0) inc = up;
    }
    if (lane == 63) s_a[wave] = inc;
    __syncthreads();
    int before = carry, all = carry;
    for (int w = 0; w < VS_WAVES; ++w) {
      const int t = s_a[w];
      if (t) {
        all = t;
        if (w < wave) before = t;
      }
    }
    const int speech = (inc ? inc : before) == 1 ? 1 : 0;
    s_b[tid] = speech;
    __syncthreads();
    const int prev = tid ? s_b[tid - 1] : (carry == 1 ? 1 : 0);
    carry = all;
    const int starts = i < n && speech && !prev ? 1 : 0, ends = i < n && !speech && prev ? 1 : 0;
    int total;
    const int rank = vs_scan(starts | (ends << 16), s_w, &total);          // at most 1 024 of either: the halves do not meet
    if (starts) rs[n_starts + (rank & 0xffff)] = i;
    if (ends) re[n_ends + (rank >> 16)] = i;
    n_starts += total & 0xffff, n_ends += total >> 16;
  }
  if (carry == 1 && n > 0 && tid == 0) re[n_ends] = n;                     // speech up to the last frame: n_ends == n_starts - 1
  __syncthreads();
  int K = n_starts;

  // ---- (b), (c) opening, closing; the mask
  K = vs_filter(rs, re, K, open_len, 0, n, s_w);
  K = vs_join(rs, re, K, close_len - 1, s_w, s_a, s_b);
  const int c = close_len / 2;
  K = vs_filter(rs, re, K, 1, c, n - (close_len - 1 - c), s_w);
  if (m)                                                                   // cleared above, and a barrier since; a wave per run
    for (int k = wave; k < K; k += VS_WAVES)
      for (int i = rs[k] + lane, e = re[k]; i < e; i += 64) m[i] = 1;      // 0 <= start < end <= n: made above from frame indices

  // ---- (d) the run rules of mask_to_segments
  K = vs_filter(rs, re, K, min_run, 0, n, s_w);
  K = vs_join(rs, re, K, max_gap, s_w, s_a, s_b);

  for (int k = tid; k < K; k += VS_THREADS) seg_start[q0 + k] = rs[k], seg_end[q0 + k] = re[k];   // K <= (n + 1) / 2 <= cap
  if (tid == 0) bad[g] = 0, n_segs[g] = K;
}

}  // namespace

extern "C" int sd_vad_abi_version(void) { return SD_VAD_ABI_VERSION; }

extern "C" int sd_vad_energy_grouped_f32(const float* signal, long long n_signal, const long long* first_sample, const int* n_samples,
                                         int n_groups, int win, int hop, float threshold_db, float slope, const int* first_frame, int n_frames,
                                         float* probs, int* bad, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SdVadEnergyCall c = {};
  c.n_groups = n_groups, c.n_frames = n_frames, c.win = win, c.hop = hop, c.n_signal = n_signal;
  c.threshold_db = threshold_db, c.slope = slope;
  c.table_null = !(first_sample && n_samples && first_frame && bad);
  c.frames_null = !(signal && probs);
  char why[SD_VAD_WHY];
  if (const int e = sd_vad_energy_check(c, why)) return sd_set_error(e, "%s", why);
  const unsigned tiles = n_frames > 0 ? (unsigned)(((long long)n_frames + SD_VAD_E_TILE - 1) / SD_VAD_E_TILE) : 1u;   // one for the flags alone
  hipLaunchKernelGGL(vad_energy_kernel, dim3(tiles), dim3(SD_VAD_E_THREADS), 0, stream, signal, n_signal, first_sample, n_samples, n_groups, win,
                     hop, threshold_db, slope, first_frame, n_frames, probs, bad);
  SD_CHECK_LAUNCH("vad_energy_kernel");
  return SD_OK;
}

extern "C" size_t sd_vad_segments_workspace_bytes(int seg_cap, int n_groups) { return sd_vad_workspace_bytes(seg_cap, n_groups); }

extern "C" int sd_vad_segments_grouped(const float* probs, const int* first_frame, int n_groups, int n_frames, float on, float off, int open_len,
                                       int close_len, int min_run, int max_gap, const int* first_seg, int seg_cap, int* n_segs, int* seg_start,
                                       int* seg_end, unsigned char* mask, int* bad, void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SdVadSegmentsCall c = {};
  c.n_groups = n_groups, c.n_frames = n_frames, c.seg_cap = seg_cap, c.open_len = open_len, c.close_len = close_len, c.min_run = min_run;
  c.max_gap = max_gap, c.on = on, c.off = off;
  c.table_null = !(first_frame && first_seg && n_segs && bad);
  c.probs_null = probs == nullptr;
  c.segs_null = !(seg_start && seg_end && ws);
  c.ws_misaligned = !sd_aligned16(ws);
  c.ws_bytes = ws_bytes;
  char why[SD_VAD_WHY];
  if (const int e = sd_vad_segments_check(c, why)) return sd_set_error(e, "%s", why);
  constexpr int lds = 2 * SD_VAD_S_LDS_RUNS * (int)sizeof(int);
  SD_CHECK_HIP(sd_func_max_lds(reinterpret_cast<const void*>(vad_segments_kernel), lds));
  hipLaunchKernelGGL(vad_segments_kernel, dim3((unsigned)n_groups), dim3(VS_THREADS), lds, stream, probs, first_frame, n_groups, n_frames, on, off,
                     open_len, close_len, min_run, max_gap, first_seg, seg_cap, n_segs, seg_start, seg_end, mask, bad, static_cast<int*>(ws));
  SD_CHECK_LAUNCH("vad_segments_kernel");
  return SD_OK;
}
