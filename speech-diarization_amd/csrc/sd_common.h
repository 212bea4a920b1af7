// Internal helpers shared by the HIP translation units of libsd_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include "sd_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

int sd_set_error(int code, const char* fmt, ...);
#include <atomic>
#include "sd_conv_choice.h"
// library-internal entry points
// The conv operators with the caller's tuning snapshot (sd_conv_choice.h; the public entries take their own): one ECAPA forward hands
// one snapshot to its plan and to every conv it launches.  sd_conv_gemm.hip, sd_conv_gemm_f16.hip.
int sd_conv1d_cl_f32_with(const sd_conv_args* a, sd_stream_t stream, const SdConvTuning& t, int* stat_rows);   // stat_rows: may be null
int sd_conv1d_cl_packed_f32_with(const sd_conv_args* a, const int* frame_start_dev, int B, sd_stream_t stream, const SdConvTuning& t);
int sd_seg_gemm_f32_with(const sd_conv_args* a, void* scratch, size_t scratch_bytes, sd_stream_t stream, const SdConvTuning& t);
int sd_conv1d_cl_f16_with(const sd_conv_args* a, sd_stream_t stream, const SdConvTuning& t);
int sd_conv1d_cl_split16_with(const sd_conv_args* a, sd_stream_t stream, const SdConvTuning& t);
int sd_conv_f16_decide(const sd_conv_args* a, int op, const SdConvTuning& t, SdConvChoice c[2], int* n, int* vec);   // check + choose of the two above
int sd_conv1d_cl_f32_symmetric(const sd_conv_args* a, sd_stream_t stream);   // sd_conv_gemm.hip: x == w, upper triangle + mirror
int sd_colstat_finish_rows(const float* colstat, const float* pivot, const void* y, int y_dtype, int ldy, int y_col0, int B, int T, int C, int want_std,
                           float eps, float* out, int unit_rows, sd_stream_t stream);              // sd_pool.hip: sd_colstat_finish_dt for such units
int sd_affinity_sym_f32(const float* xn, int ldx, int N, int groups, float* out, long ldo, sd_stream_t stream);                          // sd_affinity.hip
int sd_affinity_sym_split16(const void* xs, int ldx, int N, int groups, float* out, long ldo, float alpha, sd_stream_t stream);   // sd_affinity.hip
int sd_cast_f32_f16(const float* x, long n, void* y, sd_stream_t stream);           // sd_pool.hip
int sd_asp_attend_pool_scaled(const void* a1, const void* wc, const void* h, int dtype, int ldh, int B, int T, int C, int att, float eps,
                              float w_scale, float* out, sd_stream_t stream,
                              const float* rel_len = nullptr);   // sd_asp_fused.hip: sd_asp_attend_pool_lens_dt with the split weights' 2^s

// The segment map of [M][ld] activations: which rows are segment s (0 <= s < B).
//   uniform: rows s T .. s T + T (M = B T); with rel_len (device f32 [B]) only the first sd_mask_frames(rel_len[s], T) of them count
//   packed:  rows span[s] .. span[s + 1] of M in all ("Packed spans", sd_hip.h)
// The per-segment operators of sd_pool.hip and the ECAPA forward take this one description.
struct SdSegs {
  bool packed;
  int B;
  int T;                      // uniform
  const float* rel_len;       // uniform, may be null
  const int* span;            // packed: frame_start, device int32 [B + 1]
  int M;                      // packed
};
inline SdSegs sd_uniform_segs(int B, int T, const float* rel_len = nullptr) { return {false, B, T, rel_len, nullptr, 0}; }
inline SdSegs sd_packed_segs(const int* frame_start, int B, int M) { return {true, B, 0, nullptr, frame_start, M}; }
// sd_pool.hip: the launchers behind sd_seg_mean_std_*, sd_se_scale_residual_* (plus the SD_DT_SPLIT16 twin arguments of the f32-split16x3
// schedule) and sd_asp_pool_*
int sd_seg_mean_std(const void* x, int dtype, int ld, int col0, const SdSegs& sg, int C, int want_std, float eps, float* out, sd_stream_t stream);
int sd_se_scale_residual(const void* x, int ldx, const float* gate, const void* res, int ldr, int r_col0, void* y, int ldy, int y_col0,
                         const SdSegs& sg, int C, int dtype, sd_stream_t stream, void* ys = nullptr, int lds = 0, int s_col0 = 0,
                         const void* res_split = nullptr, int ld_rs = 0, int rs_col0 = 0, int write_y = 1);
int sd_asp_pool(const void* logit, int ldl, const void* h, int dtype, int ldh, const SdSegs& sg, int C, float eps, float* out, sd_stream_t stream);

// sd_conv_gemm.hip: the argument rules every conv operator shares (sd_conv_args, sd_hip.h).  On SD_OK *vec says whether the 16-byte
// epilogue stores apply.  The operator checks its own dtypes first and its grid after.
struct SdConvRule {
  const char* fn;             // the entry's name, for messages
  int gran;                   // value granularity of cin / lda / a_col0: 4, 8; 32 for the wide split form (whose operand is cin_pad wide)
  int kpad;                   // cin_pad granularity
  int store;                  // store granularity of the vector epilogue (ldo, o_col0, ldt, ld_ta, ta_col0): 4 exact f32, 8 f16 / split
  bool packed;                // packed spans: neither M % T nor the reflect check (a->T is ignored)
  bool tee_add;               // the kernel has the tee_add epilogue
  int colstat_T;              // column statistics need T >= this (SD_COLSTAT_T_128 / _256); 0: refused (SD_ERR_UNSUPPORTED)
};
int sd_check_conv(const sd_conv_args* a, const SdConvRule& r, int* vec);

#define SD_CHECK_ARG(cond, ...)                            \
  do {                                                     \
    if (!(cond)) return sd_set_error(SD_ERR_ARG, __VA_ARGS__); \
  } while (0)

#define SD_CHECK_HIP(expr)                                                              \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return sd_set_error(SD_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
  } while (0)

// Kernel launches report configuration errors through hipGetLastError.  `name` is the launch LABEL: the kernel's own name, then
// <...> for the instantiation and /... for the walk where the host chose one at run time ("conv_gemm_f32_s64_kernel<32>",
// "conv_gemm_f16_t256_kernel<f16,direct>/lockstep").  It must be a string literal (or a choice between literals): the launch log
// (sd_hip_trace.h) keeps the pointer.  With the log off a successful launch costs one relaxed atomic load.
extern std::atomic<int> sd_launch_log_state;       // sd_api.hip: bit 0 the scoped log (sd_launch_log_enable), bit 1 the whole-process census
void sd_launch_log_note(const char* label);        // sd_api.hip: host only; no device work, no synchronisation
#define SD_CHECK_LAUNCH(name)                                                           \
  do {                                                                                  \
    hipError_t e_ = hipGetLastError();                                                  \
    if (e_ != hipSuccess)                                                               \
      return sd_set_error(SD_ERR_HIP, "launch of %s failed: %s", name, hipGetErrorString(e_)); \
    if (sd_launch_log_state.load(std::memory_order_relaxed)) sd_launch_log_note(name);  \
  } while (0)

// ---- optional per-kernel timing with HIP events on the launch stream (sd_profile_* in sd_hip.h)
struct SdProfScope {
  SdProfScope(int kind, hipStream_t stream, double work);
  ~SdProfScope();
  int slot;
  hipStream_t stream;
};

// hipFuncSetAttribute(func, MaxDynamicSharedMemorySize, bytes) once per (device, kernel): thread-safe, keyed by the
// calling thread's current device, so a second GPU in the same process or two threads racing the first call
// (the reference's web UI calls the pipeline from a worker thread) both get the attribute set before the launch.
hipError_t sd_func_max_lds(const void* func, int bytes);

// A/B switches (SD_F16_KERNEL, SD_RES2_FUSED, ...) re-route kernels and exist for measurements only: they are read ONLY when the
// process also sets SD_EXPERIMENT=1, so a stray SD_* variable cannot change which kernels a product run uses.
static inline const char* sd_experiment_env(const char* name) {
  static const bool on = [] { const char* e = getenv("SD_EXPERIMENT"); return e && e[0] == '1' && e[1] == 0; }();
  return on ? getenv(name) : nullptr;
}

static inline bool sd_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// The value an f32 activation / operand takes on its way into an SD_DT_SPLIT16 pair (hi = f16(w), lo = f16(w - hi)): clamped to the
// f16 range, NaN kept (v_med3_f32 alone returns min3 of its operands for a NaN, i.e. -65504: a NaN would be laundered into a
// finite value).  Every split site uses this, so a producer that writes split halves gives the bits sd_split16_pack_f32 would.
__device__ __forceinline__ float sd_split16_clamp(float v) {
  const float c = __builtin_amdgcn_fmed3f(v, -65504.f, 65504.f);
  return v != v ? v : c;
}

// max(x, lo) that KEEPS a NaN x (ReLU: lo = 0; identity: lo = -inf).  v_max_f32 returns the other operand for a NaN, so a NaN activation
// (say the features sd_fbank writes for an utterance with a NaN sample) would become 0 in the first ReLU and the segment would leave the
// network with a plausible finite embedding; torch's relu / clamp propagate it [REF speech_encode.py:77 via speechbrain's TDNNBlock].
// One v_cmp + v_cndmask instead of one v_max per output element (-DSD_RELU_VMAX: the old form, for A/B timing only).
__device__ __forceinline__ float sd_max_keep_nan(float x, float lo) {
#ifdef SD_RELU_VMAX
  return fmaxf(x, lo);
#else
  return x < lo ? lo : x;
#endif
}

// Relative lengths (speechbrain's wav_lens: the share of the padded row that is signal) -> frames of a row of T frames.  Both counts
// start from p = f32(rel * T), the f32 product torch forms (unpinned restatement of speechbrain 1.0):
//   sd_norm_frames  InputNormalization(norm_type="sentence"): actual_size = torch.round(lengths * T) -> round half to even, clamped to [0, T]
//   sd_mask_frames  length_to_mask(lengths * L, max_len=L): #{t in [0, T) : float(t) < p} = min(T, ceil(p)) (SE squeeze, pooling)
// They differ by one when frac(p) is in (0, 0.5) (p = 100.3: 100 and 101): speechbrain's behaviour, kept.  A NaN or p <= 0 gives 0.
// This is the ONE statement of the rule on the device; every masked kernel computes its row's counts from rel_len[b] with it.
__host__ __device__ __forceinline__ int sd_norm_frames(float rel, int T) {
  const float r = rintf(rel * (float)T);
  return r >= (float)T ? T : (r > 0.f ? (int)r : 0);
}
__host__ __device__ __forceinline__ int sd_mask_frames(float rel, int T) {
  const float c = ceilf(rel * (float)T);
  return c >= (float)T ? T : (c > 0.f ? (int)c : 0);
}

// Packed spans (sd_hip.h): the span that owns row m = the largest s < B with frame_start[s] <= m (0 if there is none).  Reads
// frame_start[1 .. B - 1] only and returns an s in [0, B) for ANY table, so a malformed one gives wrong numbers, never a wild index.
__device__ __forceinline__ int sd_span_of(const int* frame_start, int B, int m) {
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (frame_start[mid] <= m) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ float sd_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float sd_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// <a, b> / (|a| |b| + eps) of two rows of D floats, by one wave (every lane calls it and every lane gets the value): lane l adds the
// products of the elements l, l + 64, ... in that order, then the 64 partial sums meet in the butterfly of sd_wave_sum.  The ONE
// statement of the pair cosine on the device: adjacent_cosine_kernel (sd_pool.hip) and scd_split_kernel (scd/sd_scd.hip) both call
// it, so the two give the same bits for the same rows and eps.  Which operations are fused is WRITTEN here and not left to the
// compiler, which contracts a * b + c in one kernel and not in another: the three sums are fused multiply-adds, the denominator is a
// rounded product plus eps (what adjacent_cosine_kernel compiled to before the statement was shared).
__device__ __forceinline__ float sd_wave_pair_cosine(const float* a, const float* b, int D, float eps, int lane) {
#pragma clang fp contract(off)
  float dot = 0.f, na = 0.f, nb = 0.f;
  for (int d = lane; d < D; d += 64) {
    dot = __builtin_fmaf(a[d], b[d], dot);
    na = __builtin_fmaf(a[d], a[d], na);
    nb = __builtin_fmaf(b[d], b[d], nb);
  }
  dot = sd_wave_sum(dot); na = sd_wave_sum(na); nb = sd_wave_sum(nb);
  const float nn = sqrtf(na) * sqrtf(nb);
  return dot / (nn + eps);
}
