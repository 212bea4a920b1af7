// The N x N operator of the spectral steps (include/sd_hip_spectral.h): row sums of max(K, 0) and
//   Y = diag(scale) . max(K, 0) . diag(scale) . V,   V a block of 8 .. 32 vectors,
// read from the f32 affinity as it lies: N^2 x 4 bytes streamed once per pass, b / 2 flop per byte.
//
// Apply kernel.  A workgroup is 4 waves and owns 128 rows (32 per wave = two 16-row groups) and a run of 256-column chunks.
// * A operand = the K tile, memory -> registers, no LDS: for v_mfma_f32_16x16x4_f32 lane (r = lane % 16, q = lane / 16) holds
//   A[r][k = q].  The lane loads 16 bytes of row r at columns c + 4 q .. + 3 and feeds component t to MFMA t, which therefore sums
//   k in {c + 4 q + t : q}; four such loads per 64-column step cover 16 rows x 256 contiguous bytes.  The clip (v_max) and the zero
//   diagonal are applied to the registers.  The loads of the next 64-column step are issued before the MFMAs of the current one.
// * B operand = the panel W[k][c] = scale[k] V[k][c] of the chunk, staged TRANSPOSED in LDS ([c][k], row stride 260 floats) so that
//   one ds_read_b128 at [c = r][k = 4 q ..] gives the B values of the same four MFMAs in the same k permutation.  Columns b .. 16 NJ
//   of the panel and rows past N are zero.  A wave reuses each B read for both of its row groups.
// * Partial sums [split][N][b] go to the workspace; apply_finish_kernel adds them in split order and applies scale[i] (the way
//   sd_seg_gemm_f32 keeps its split-K reproducible).
#include <hip/hip_runtime.h>

#include "sd_common.h"
#include "sd_hip_spectral.h"

namespace {

constexpr int AP_ROWS = 128;              // rows of a workgroup
constexpr int AP_CK = 256;                // columns of a staged chunk
constexpr int AP_STEP = 64;               // columns of one register step
constexpr int AP_LDW = AP_CK + 4;         // LDS row stride of the transposed panel, floats
constexpr int AP_TARGET_WG = 2048;        // workgroups wanted: 8 per CU, four rounds of the two resident ones
constexpr int AP_MIN_PER = 2;             // but at least 512 columns each where the matrix has them: the partial sums stay small next to K

struct ApSplit {
  int chunks, splits, per;                // 256-column chunks in all, column splits, chunks per split
};
inline ApSplit ap_split(int N) {
  ApSplit s;
  s.chunks = (N + AP_CK - 1) / AP_CK;
  const int rb = (N + AP_ROWS - 1) / AP_ROWS;
  int want = AP_TARGET_WG / rb;
  want = want < 1 ? 1 : want;
  want = want > s.chunks ? s.chunks : want;
  s.per = (s.chunks + want - 1) / want;
  if (s.per < AP_MIN_PER) s.per = s.chunks < AP_MIN_PER ? s.chunks : AP_MIN_PER;
  s.splits = (s.chunks + s.per - 1) / s.per;
  return s;
}
inline bool ap_block_ok(int b) { return b == 8 || b == 16 || b == 24 || b == 32; }

// 16 bytes of a K row at columns c .. c + 3 (c % 4 == 0), zeros past column N; clipped at 0
template <bool VEC>
__device__ __forceinline__ f32x4 ap_load4(const float* __restrict__ row, int c, int N) {
  f32x4 v;
  if (VEC && c + 3 < N) {
    v = *reinterpret_cast<const f32x4*>(row + c);
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = c + t < N ? row[c + t] : 0.f;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) v[t] = fmaxf(v[t], 0.f);
  return v;
}

template <int NJ, bool VEC>
__global__ __launch_bounds__(256, 2) void affinity_apply_kernel(const float* __restrict__ K, const int N, const long ld, const int zero_diag,
                                                                const float* __restrict__ scale, const float* __restrict__ V, const int ldv,
                                                                const int b, float* __restrict__ part, const int chunks, const int per) {
  __shared__ __attribute__((aligned(16))) float wt[16 * NJ * AP_LDW];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int row0 = blockIdx.x * AP_ROWS + wid * 32;
  const int ch0 = blockIdx.y * per;
  const int ch1 = ch0 + per < chunks ? ch0 + per : chunks;

  const float* rowp[2];
  int myrow[2];
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    myrow[g] = row0 + 16 * g + fr;
    rowp[g] = K + (size_t)(myrow[g] < N ? myrow[g] : N - 1) * ld;       // rows past N read row N - 1 and are not stored
  }

  f32x4 acc[2][NJ];
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[g][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  f32x4 a[2][2][4];                       // [buffer][row group][16-column piece]
  auto load = [&](f32x4 (&dst)[2][4], int c0) {
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = c0 + 16 * u + 4 * fq;
        f32x4 v = ap_load4<VEC>(rowp[g], c, N);
        if (zero_diag) {
          const int d = myrow[g] - c;
#pragma unroll
          for (int t = 0; t < 4; ++t) v[t] = d == t ? 0.f : v[t];
        }
        dst[g][u] = v;
      }
  };
  auto compute = [&](const f32x4 (&src)[2][4], int koff) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(&wt[(16 * j + fr) * AP_LDW + koff + 16 * u + 4 * fq]);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int g = 0; g < 2; ++g) acc[g][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(src[g][u][t], bv[t], acc[g][j], 0, 0, 0);
      }
  };

  if (ch0 < ch1) load(a[0], ch0 * AP_CK);
  for (int ch = ch0; ch < ch1; ++ch) {
    const int c0 = ch * AP_CK;
    __syncthreads();                      // every wave is done with the previous panel
    {
      const int j = tid & 31;
      for (int k = tid >> 5; k < AP_CK; k += 8) {
        const int gk = c0 + k;
        const float w = (j < b && gk < N) ? V[(size_t)gk * ldv + j] * scale[gk] : 0.f;
        if (j < 16 * NJ) wt[j * AP_LDW + k] = w;
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < AP_CK / AP_STEP; ++s) {
      if (s + 1 < AP_CK / AP_STEP) load(a[(s + 1) & 1], c0 + (s + 1) * AP_STEP);
      else if (ch + 1 < ch1) load(a[0], c0 + AP_CK);
      compute(a[s & 1], s * AP_STEP);
    }
  }

  // acc[g][j][r] = partial of row row0 + 16 g + 4 fq + r, column 16 j + fr
  float* const out = part + (size_t)blockIdx.y * N * b;
#pragma unroll
  for (int g = 0; g < 2; ++g)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + 16 * g + 4 * fq + r, col = 16 * j + fr;
        if (row < N && col < b) out[(size_t)row * b + col] = acc[g][j][r];
      }
}

__global__ __launch_bounds__(256) void apply_finish_kernel(const float* __restrict__ part, const int splits, const int N, const int b,
                                                           const float* __restrict__ scale, float* __restrict__ Y, const int ldy) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const long total = (long)N * b;
  if (idx >= total) return;
  const int i = (int)(idx / b), c = (int)(idx % b);
  float s = part[idx];
  for (int p = 1; p < splits; ++p) s += part[(size_t)p * total + idx];
  Y[(size_t)i * ldy + c] = scale[i] * s;
}

__global__ __launch_bounds__(256) void affinity_degree_kernel(const float* __restrict__ K, const int N, const long ld, const int zero_diag,
                                                              float* __restrict__ deg) {
  __shared__ float wsum[4];
  const int i = blockIdx.x;
  const int tid = threadIdx.x;
  const float* __restrict__ row = K + (size_t)i * ld;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  int j = tid;
  for (; j + 768 < N; j += 1024) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = j + 256 * u;
      const float v = fmaxf(row[c], 0.f);
      s[u] += (zero_diag && c == i) ? 0.f : v;
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = j + 256 * u;
    if (c < N) {
      const float v = fmaxf(row[c], 0.f);
      s[u] += (zero_diag && c == i) ? 0.f : v;
    }
  }
  float t = sd_wave_sum((s[0] + s[1]) + (s[2] + s[3]));
  if ((tid & 63) == 0) wsum[tid >> 6] = t;
  __syncthreads();
  if (tid == 0) deg[i] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

}  // namespace

extern "C" int sd_spectral_abi_version(void) { return SD_SPECTRAL_ABI_VERSION; }

extern "C" int sd_affinity_degree_f32(const float* K, int N, long ld, int zero_diag, float* deg, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SD_CHECK_ARG(N > 0 && ld >= N, "sd_affinity_degree_f32: N=%d ld=%ld", N, ld);
  SD_CHECK_ARG(K && deg, "sd_affinity_degree_f32: null pointer");
  hipLaunchKernelGGL(affinity_degree_kernel, dim3((unsigned)N), dim3(256), 0, stream, K, N, ld, zero_diag != 0, deg);
  SD_CHECK_LAUNCH("affinity_degree_kernel");
  return SD_OK;
}

extern "C" size_t sd_affinity_apply_workspace_bytes(int N, int b) {
  if (N <= 0 || !ap_block_ok(b)) return 0;
  const size_t bytes = (size_t)ap_split(N).splits * N * b * sizeof(float);
  return (bytes + 255) & ~(size_t)255;
}

extern "C" int sd_affinity_apply_f32(const float* K, int N, long ld, int zero_diag, const float* scale, const float* V, int ldv, int b,
                                     float* Y, int ldy, void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  if (!ap_block_ok(b)) return sd_set_error(SD_ERR_UNSUPPORTED, "sd_affinity_apply_f32: b=%d, supported block widths are 8, 16, 24, 32", b);
  SD_CHECK_ARG(N > 0 && ld >= N && ldv >= b && ldy >= b, "sd_affinity_apply_f32: N=%d ld=%ld ldv=%d ldy=%d b=%d", N, ld, ldv, ldy, b);
  SD_CHECK_ARG(K && scale && V && Y && ws, "sd_affinity_apply_f32: null pointer");
  SD_CHECK_ARG(sd_aligned16(ws), "sd_affinity_apply_f32: workspace is not 16-byte aligned");
  const size_t need = sd_affinity_apply_workspace_bytes(N, b);
  if (ws_bytes < need)
    return sd_set_error(SD_ERR_WORKSPACE, "sd_affinity_apply_f32: workspace of %zu bytes, N=%d b=%d needs %zu", ws_bytes, N, b, need);
  const ApSplit sp = ap_split(N);
  const int rb = (N + AP_ROWS - 1) / AP_ROWS;
  const bool vec = sd_aligned16(K) && ld % 4 == 0;
  float* part = static_cast<float*>(ws);
  const dim3 grid((unsigned)rb, (unsigned)sp.splits);
#define SD_AP_LAUNCH(NJ, VEC)                                                                                                        \
  hipLaunchKernelGGL((affinity_apply_kernel<NJ, VEC>), grid, dim3(256), 0, stream, K, N, ld, zero_diag != 0, scale, V, ldv, b, part, \
                     sp.chunks, sp.per)
  if (b <= 16) {
    if (vec) SD_AP_LAUNCH(1, true);
    else SD_AP_LAUNCH(1, false);
  } else {
    if (vec) SD_AP_LAUNCH(2, true);
    else SD_AP_LAUNCH(2, false);
  }
#undef SD_AP_LAUNCH
  // <column blocks of 16 per thread, 16-byte or scalar loads of K>
  SD_CHECK_LAUNCH(b <= 16 ? (vec ? "affinity_apply_kernel<1,vec>" : "affinity_apply_kernel<1,scalar>")
                          : (vec ? "affinity_apply_kernel<2,vec>" : "affinity_apply_kernel<2,scalar>"));
  const long total = (long)N * b;
  hipLaunchKernelGGL(apply_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, part, sp.splits, N, b, scale, Y, ldy);
  SD_CHECK_LAUNCH("apply_finish_kernel");
  return SD_OK;
}
