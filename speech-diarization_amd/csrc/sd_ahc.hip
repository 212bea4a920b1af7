// Average-linkage cosine clustering without the N x N matrix (include/sd_hip_ahc.h): a cluster is the sum of its unit rows and its
// size, score(A, B) = <s_A, s_B> / (|A| |B|).  One round = the nearest neighbour of every active cluster (Gram with argmax, nothing
// of the Gram matrix is stored) + the merge of every reciprocal pair above the threshold.
//
// Nearest kernel.  A workgroup is 4 waves as 2 x 2 and owns one 128 x 128 tile on or above the diagonal; a wave owns 64 x 64 = 4 x 4
// accumulators of v_mfma_f32_16x16x4_f32 (the arithmetic and the accumulator layout of the exact form of sd_affinity.hip).
// * Operands: the 128 rows of the tile's row block and of its column block, 32 k at a time, memory -> registers -> LDS (row stride
//   36 floats); the loads of the next 32 k are issued before the MFMAs of the current ones.  A lane reads four consecutive k
//   (ds_read_b128) at chunk fq = lane / 16 and feeds element r to MFMA r, which sums k in {4 fq + r}; both operands use the same
//   permutation and every tile walks k in the same order.  Columns [d, ld) are not read: the last group of four is loaded element
//   by element, zeros past d.
// * Epilogue from registers: acc[i][j][r] = <row rbase + 16 i + 4 fq + r, row cbase + 16 j + fr>, scaled by (inv[row] · inv[col]).
//   Row maxima: over j in the lane, over fr across the 16-lane row, over the two waves of a row through LDS -> slot [J + 1] of row
//   block I.  Column maxima (the row maxima of the mirrored tile, from the same accumulators): over i, r in the lane, over fq
//   across lanes 16 / 32 apart, over the two waves of a column -> slot [I] of row block J.  The diagonal tile keeps col > row for
//   the first and row < col for the second.  Among equal scores the lowest index wins at every step.
// * ahc_nearest_finish_kernel walks the T + 1 slots of a row in ascending order with a strict >.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "sd_common.h"
#include "sd_hip_ahc.h"

namespace {

constexpr int AH_T = 128;                 // tile edge
constexpr int AH_KC = 32;                 // k of one staged chunk
constexpr int AH_LDS = AH_KC + 4;         // LDS row stride, floats: rows stay 16-byte aligned, consecutive rows shift by 4 banks
constexpr int AH_MAX_D = 1024;
constexpr int AH_MAX_TILES = 65535;       // grid.y

// columns c .. c + 3 of a row (c % 4 == 0), zeros from column d on; nothing at or past d is read
__device__ __forceinline__ f32x4 ah_load4(const float* __restrict__ row, int c, int d) {
  f32x4 v;
  if (c + 3 < d) {
    v = *reinterpret_cast<const f32x4*>(row + c);
  } else {
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = c + t < d ? row[c + t] : 0.f;
  }
  return v;
}

// (bv, bi) <- the better of it and (v, i): the larger score, the lower index among equal scores
__device__ __forceinline__ void ah_take(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

__global__ __launch_bounds__(256, 2) void ahc_nearest_kernel(const float* __restrict__ sums, const long ld, const int n, const int d,
                                                             const float* __restrict__ inv_count, float* __restrict__ ws_val,
                                                             int* __restrict__ ws_idx, const int npad) {
  const int tj = blockIdx.x, ti = blockIdx.y;
  if (ti > tj) return;                      // workgroup-uniform: below the diagonal
  __shared__ __attribute__((aligned(16))) float lds[2 * AH_T * AH_LDS];
  __shared__ float red_v[2][AH_T];
  __shared__ int red_i[2][AH_T];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;

  // staging role: thread (r0 = tid / 8, g = tid % 8) moves columns 4 g .. 4 g + 3 of rows r0 + 32 i of both operands
  const int g = tid & 7, r0 = tid >> 3;
  const float* pa[4];
  const float* pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int m = ti * AH_T + r0 + 32 * i;
    int c = tj * AH_T + r0 + 32 * i;
    m = m < n ? m : n - 1;                  // rows past n read row n - 1; their scores are never taken
    c = c < n ? c : n - 1;
    pa[i] = sums + (size_t)m * ld;
    pb[i] = sums + (size_t)c * ld;
  }
  f32x4 ra[4], rb[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = ah_load4(pa[i], k0 + 4 * g, d);
      rb[i] = ah_load4(pb[i], k0 + 4 * g, d);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float* const a_base = lds + (wm * 64 + fr) * AH_LDS;
  const float* const b_base = lds + (AH_T + wn * 64 + fr) * AH_LDS;
  const int nk = (d + AH_KC - 1) / AH_KC;
  fetch(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                        // every wave is done with the previous chunk
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<f32x4*>(&lds[(r0 + 32 * i) * AH_LDS + 4 * g]) = ra[i];
      *reinterpret_cast<f32x4*>(&lds[(AH_T + r0 + 32 * i) * AH_LDS + 4 * g]) = rb[i];
    }
    __syncthreads();
    if (kt + 1 < nk) fetch((kt + 1) * AH_KC);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int off = 16 * h + 4 * fq;
      f32x4 av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const f32x4*>(a_base + i * 16 * AH_LDS + off);
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const f32x4*>(b_base + j * 16 * AH_LDS + off);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][r], bv[j][r], acc[i][j], 0, 0, 0);
    }
  }

  // scores: acc[i][j][r] · (inv[row] · inv[col]); the product of the two factors commutes, so the mirrored element is the same bits
  const int rbase = ti * AH_T + wm * 64, cbase = tj * AH_T + wn * 64;
  const bool diag = ti == tj;
  int col[4];
  float invc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    col[j] = cbase + 16 * j + fr;
    invc[j] = col[j] < n ? inv_count[col[j]] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rbase + 16 * i + 4 * fq + r;
      const float invr = row < n ? inv_count[row] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j][r] *= invr * invc[j];
    }

  // row maxima over the tile's columns -> slot tj + 1 of row block ti
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rbase + 16 * i + 4 * fq + r;
      float bv = -INFINITY;
      int bi = INT_MAX;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (col[j] < n && (!diag || col[j] > row)) ah_take(bv, bi, acc[i][j][r], col[j]);
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        ah_take(bv, bi, ov, oi);
      }
      if (fr == 0) {
        red_v[wn][wm * 64 + 16 * i + 4 * fq + r] = bv;
        red_i[wn][wm * 64 + 16 * i + 4 * fq + r] = bi;
      }
    }
  __syncthreads();
  if (tid < AH_T) {
    float bv = red_v[0][tid];
    int bi = red_i[0][tid];
    ah_take(bv, bi, red_v[1][tid], red_i[1][tid]);
    const size_t at = (size_t)(tj + 1) * npad + (size_t)ti * AH_T + tid;
    ws_val[at] = bv;
    ws_idx[at] = bi == INT_MAX ? -1 : bi;
  }
  __syncthreads();

  // column maxima over the tile's rows = row maxima of the mirrored tile -> slot ti of row block tj
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float bv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rbase + 16 * i + 4 * fq + r;
        if (row < n && (!diag || row < col[j])) ah_take(bv, bi, acc[i][j][r], row);
      }
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      ah_take(bv, bi, ov, oi);
    }
    if (fq == 0) {
      red_v[wm][wn * 64 + 16 * j + fr] = bv;
      red_i[wm][wn * 64 + 16 * j + fr] = bi;
    }
  }
  __syncthreads();
  if (tid < AH_T) {
    float bv = red_v[0][tid];
    int bi = red_i[0][tid];
    ah_take(bv, bi, red_v[1][tid], red_i[1][tid]);
    const size_t at = (size_t)ti * npad + (size_t)tj * AH_T + tid;
    ws_val[at] = bv;
    ws_idx[at] = bi == INT_MAX ? -1 : bi;
  }
}

// the slots of row i in ascending column order, strict >: the lowest index among equal maxima
__global__ __launch_bounds__(256) void ahc_nearest_finish_kernel(const float* __restrict__ ws_val, const int* __restrict__ ws_idx,
                                                                 const int slots, const int npad, const int n, int* __restrict__ nn,
                                                                 float* __restrict__ best) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float bv = -INFINITY;
  int bi = -1;
  for (int s = 0; s < slots; ++s) {
    const float v = ws_val[(size_t)s * npad + i];
    if (v > bv) {
      bv = v;
      bi = ws_idx[(size_t)s * npad + i];
    }
  }
  nn[i] = bi;
  best[i] = bv;
}

// one workgroup per row r: the lower row of a pair adds the upper one in, the upper row points at the lower, every other row at itself
__global__ __launch_bounds__(64) void ahc_merge_kernel(float* __restrict__ sums, const long ld, const int n, const int d,
                                                       float* __restrict__ count, float* __restrict__ inv_count,
                                                       const int* __restrict__ nn, const float* __restrict__ best, const float cos_thr,
                                                       int* __restrict__ target, int* __restrict__ n_merged) {
  const int r = blockIdx.x;
  const int tid = threadIdx.x;
  const int p = nn[r];
  bool paired = false;
  if (p >= 0 && p < n && p != r && nn[p] == r) paired = best[r < p ? r : p] > cos_thr;
  if (!paired || r > p) {
    if (tid == 0) target[r] = paired ? p : r;
    return;
  }
  float* const a = sums + (size_t)r * ld;
  const float* const b = sums + (size_t)p * ld;       // row p is written by nobody in this launch
  for (int c = tid; c < d; c += 64) a[c] += b[c];
  if (tid == 0) {
    const float c = count[r] + count[p];
    count[r] = c;
    inv_count[r] = __fdiv_rn(1.f, c);
    target[r] = r;
    atomicAdd(n_merged, 1);
  }
}

inline int ah_tiles(int n) { return (n + AH_T - 1) / AH_T; }

}  // namespace

extern "C" int sd_ahc_abi_version(void) { return SD_AHC_ABI_VERSION; }

extern "C" size_t sd_ahc_nearest_workspace_bytes(int n, int d) {
  if (n <= 0 || d <= 0 || d > AH_MAX_D) return 0;
  const size_t nt = (size_t)ah_tiles(n);
  return (nt + 1) * nt * AH_T * (sizeof(float) + sizeof(int));
}

extern "C" int sd_ahc_nearest_f32(const float* sums, long ld, int n, int d, const float* inv_count, int* nn, float* best, void* ws,
                                  size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SD_CHECK_ARG(n > 0 && d > 0 && ld >= d, "sd_ahc_nearest_f32: n=%d d=%d ld=%ld", n, d, ld);
  if (d > AH_MAX_D) return sd_set_error(SD_ERR_UNSUPPORTED, "sd_ahc_nearest_f32: d=%d, at most %d columns are supported", d, AH_MAX_D);
  SD_CHECK_ARG(sums && inv_count && nn && best && ws, "sd_ahc_nearest_f32: null pointer");
  SD_CHECK_ARG(sd_aligned16(sums) && ld % 4 == 0, "sd_ahc_nearest_f32: sums must be 16-byte aligned with ld %% 4 == 0 (ld=%ld)", ld);
  SD_CHECK_ARG(sd_aligned16(ws), "sd_ahc_nearest_f32: workspace is not 16-byte aligned");
  const int nt = ah_tiles(n);
  if (nt > AH_MAX_TILES) return sd_set_error(SD_ERR_UNSUPPORTED, "sd_ahc_nearest_f32: n=%d, at most %d rows are supported", n, AH_MAX_TILES * AH_T);
  const size_t need = sd_ahc_nearest_workspace_bytes(n, d);
  if (ws_bytes < need)
    return sd_set_error(SD_ERR_WORKSPACE, "sd_ahc_nearest_f32: workspace of %zu bytes, n=%d d=%d needs %zu", ws_bytes, n, d, need);
  const int npad = nt * AH_T;
  const int slots = nt + 1;
  float* ws_val = static_cast<float*>(ws);
  int* ws_idx = reinterpret_cast<int*>(ws_val + (size_t)slots * npad);
  hipLaunchKernelGGL(ahc_nearest_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, stream, sums, ld, n, d, inv_count, ws_val, ws_idx,
                     npad);
  SD_CHECK_LAUNCH("ahc_nearest_kernel");
  hipLaunchKernelGGL(ahc_nearest_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws_val, ws_idx, slots, npad, n, nn,
                     best);
  SD_CHECK_LAUNCH("ahc_nearest_finish_kernel");
  return SD_OK;
}

extern "C" int sd_ahc_merge_f32(float* sums, long ld, int n, int d, float* count, float* inv_count, const int* nn, const float* best,
                                float cos_thr, int* target, int* n_merged, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SD_CHECK_ARG(n > 0 && d > 0 && ld >= d, "sd_ahc_merge_f32: n=%d d=%d ld=%ld", n, d, ld);
  SD_CHECK_ARG(sums && count && inv_count && nn && best && target && n_merged, "sd_ahc_merge_f32: null pointer");
  SD_CHECK_ARG(sd_aligned16(sums) && ld % 4 == 0, "sd_ahc_merge_f32: sums must be 16-byte aligned with ld %% 4 == 0 (ld=%ld)", ld);
  SD_CHECK_HIP(hipMemsetAsync(n_merged, 0, sizeof(int), stream));
  hipLaunchKernelGGL(ahc_merge_kernel, dim3((unsigned)n), dim3(64), 0, stream, sums, ld, n, d, count, inv_count, nn, best, cos_thr, target,
                     n_merged);
  SD_CHECK_LAUNCH("ahc_merge_kernel");
  return SD_OK;
}
