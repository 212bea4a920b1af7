// Average-linkage cosine clustering without the N x N matrix (include/sd_hip_ahc.h): a cluster is the sum of its unit rows and its
// size, score(A, B) = <s_A, s_B> / (|A| |B|).  One round = the nearest neighbour of every active cluster (Gram with argmax, nothing
// of the Gram matrix is stored) + the merge of every reciprocal pair above the threshold.
//
// Nearest kernel: one 128 x 128 tile on or above the diagonal per workgroup; the tile, the symmetric argmax and the walk of its slots
// (ahc_nearest_finish_kernel) are sd_gram_tile.h's.  Its own part is the weight: acc[i][j][r] scaled by (inv[row] · inv[col]).
#include <hip/hip_runtime.h>

#include "sd_common.h"
#include "sd_gram_tile.h"
#include "sd_hip_ahc.h"

namespace {

__global__ __launch_bounds__(256, 2) void ahc_nearest_kernel(const float* __restrict__ sums, const long ld, const int n, const int d,
                                                             const float* __restrict__ inv_count, float* __restrict__ ws_val,
                                                             int* __restrict__ ws_idx, const int npad) {
  const int tj = blockIdx.x, ti = blockIdx.y;
  if (ti > tj) return;                      // workgroup-uniform: below the diagonal
  __shared__ __attribute__((aligned(16))) float lds[2 * GT_T * GT_LDS];
  __shared__ float red_v[2][GT_T];
  __shared__ int red_i[2][GT_T];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;

  f32x4 acc[4][4];
  gt_tile(sums, ld, n, d, ti, tj, lds, acc, tid, wm, wn, fr, fq);

  // scores: acc[i][j][r] · (inv[row] · inv[col]); the product of the two factors commutes, so the mirrored element is the same bits
  const int rbase = ti * GT_T + wm * 64, cbase = tj * GT_T + wn * 64;
  float invc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = cbase + 16 * j + fr;
    invc[j] = col < n ? inv_count[col] : 0.f;
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

  gt_sym_argmax(acc, [](int, int, int) { return true; }, ti, tj, tj + 1, ti, n, npad, red_v, red_i, ws_val, ws_idx, tid, wm, wn, fr, fq);
}

__global__ __launch_bounds__(256) void ahc_nearest_finish_kernel(const float* __restrict__ ws_val, const int* __restrict__ ws_idx,
                                                                 const int slots, const int npad, const int n, int* __restrict__ nn,
                                                                 float* __restrict__ best) {
  gt_finish(ws_val, ws_idx, slots, npad, n, nn, best, blockIdx.x * 256 + threadIdx.x);
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

}  // namespace

extern "C" int sd_ahc_abi_version(void) { return SD_AHC_ABI_VERSION; }

extern "C" size_t sd_ahc_nearest_workspace_bytes(int n, int d) { return sd_rows_workspace_bytes(SD_ROWS_SYM, n, d, 1, GT_MAX_D); }

extern "C" int sd_ahc_nearest_f32(const float* sums, long ld, int n, int d, const float* inv_count, int* nn, float* best, void* ws,
                                  size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const SdRowsCall c = {"sd_ahc_nearest_f32", "sums", SD_ROWS_SYM, n, d, ld, 1, GT_MAX_D};
  if (const int e = sd_rows_refused(c, sums, !(sums && inv_count && nn && best && ws), ws, ws_bytes)) return e;
  const int nt = gt_tiles(n);
  const GtSymWs w = gt_sym_ws(ws, nt, nt + 1);
  hipLaunchKernelGGL(ahc_nearest_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, stream, sums, ld, n, d, inv_count, w.val, w.idx,
                     w.npad);
  SD_CHECK_LAUNCH("ahc_nearest_kernel");
  hipLaunchKernelGGL(ahc_nearest_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w.val, w.idx, w.slots, w.npad, n, nn,
                     best);
  SD_CHECK_LAUNCH("ahc_nearest_finish_kernel");
  return SD_OK;
}

extern "C" int sd_ahc_merge_f32(float* sums, long ld, int n, int d, float* count, float* inv_count, const int* nn, const float* best,
                                float cos_thr, int* target, int* n_merged, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const SdRowsCall c = {"sd_ahc_merge_f32", "sums", SD_ROWS_ONLY, n, d, ld, 1, INT_MAX};      // one thread walks a row: no limit on d
  if (const int e = sd_rows_refused(c, sums, !(sums && count && inv_count && nn && best && target && n_merged))) return e;
  SD_CHECK_HIP(hipMemsetAsync(n_merged, 0, sizeof(int), stream));
  hipLaunchKernelGGL(ahc_merge_kernel, dim3((unsigned)n), dim3(64), 0, stream, sums, ld, n, d, count, inv_count, nn, best, cos_thr, target,
                     n_merged);
  SD_CHECK_LAUNCH("ahc_merge_kernel");
  return SD_OK;
}
