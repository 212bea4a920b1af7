// The nearest pass of average-linkage clustering for MANY recordings at once (include/sd_hip_ahc.h, sd_ahc_nearest_grouped_f32): the
// rows of all recordings stand one after another, `group` names the recording of every row (non-decreasing), and only a pair of rows
// of one recording is a candidate.  The tile, the symmetric argmax and the walk of the slots are sd_gram_tile.h's, the weight is
// ahc_nearest_kernel's (sd_ahc.hip): a recording's scores are the bits it gets when it is clustered alone.
//
// The walk is a band.  Rows r < c of one group lie at most max_group - 1 apart, so tile (ti, tj) can hold a candidate only for
// k = tj - ti <= W = min(T - 1, ceil((max_group - 1) / 128)), T = ceil(n / 128).  Grid (T, W + 1): workgroup (ti, k) owns tile
// (ti, ti + k).  A row block has 2 W + 2 slots, in ascending column order:
//   slot W - k      the column maxima of tile (tj - k, tj), k = W .. 0 (the tiles to its left, then the diagonal tile's row > col half)
//   slot W + 1 + k  the row maxima of tile (ti, ti + k), k = 0 .. W (the diagonal tile's col > row half, then the tiles to its right)
// The left slot [W - k] of a row block b < k has no tile: there are k of them for every k, as many as there are workgroups with
// ti + k >= T.  Workgroup (ti, k) with ti + k >= T therefore owns the empty tile (ti, (ti + k) mod T): it writes (-inf, -1) into its
// row slot and into left slot [W - k] of row block ti + k - T.  Every slot of every row block is written exactly once per launch.
#include <hip/hip_runtime.h>

#include "sd_common.h"
#include "sd_gram_tile.h"
#include "sd_hip_ahc.h"

namespace {

__global__ __launch_bounds__(256, 2) void ahc_nearest_grouped_kernel(const float* __restrict__ sums, const long ld, const int n, const int d,
                                                                     const float* __restrict__ inv_count, const int* __restrict__ group,
                                                                     float* __restrict__ ws_val, int* __restrict__ ws_idx, const int npad,
                                                                     const int nt, const int band) {
  const int ti = blockIdx.x, k = blockIdx.y;
  const int slot_row = band + 1 + k, slot_col = band - k;
  const int tid = threadIdx.x;
  int tj = ti + k;
  // workgroup-uniform: a tile past the last one, or a row block and a column block that share no group (group is non-decreasing:
  // the largest group of the rows is that of the last row, the smallest of the columns that of the first column)
  bool empty = tj >= nt;
  if (empty) tj -= nt;
  else if (k > 0) empty = group[ti * GT_T + GT_T - 1] != group[tj * GT_T];
  if (empty) {
    if (tid < GT_T) {
      const size_t at = (size_t)slot_row * npad + (size_t)ti * GT_T + tid;
      ws_val[at] = -INFINITY;
      ws_idx[at] = -1;
    } else {
      const size_t at = (size_t)slot_col * npad + (size_t)tj * GT_T + (tid - GT_T);
      ws_val[at] = -INFINITY;
      ws_idx[at] = -1;
    }
    return;
  }
  __shared__ __attribute__((aligned(16))) float lds[2 * GT_T * GT_LDS];
  __shared__ float red_v[2][GT_T];
  __shared__ int red_i[2][GT_T];
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;

  // the groups of the tile's 128 rows ([0]) and 128 columns ([1]): one load per thread, issued before the K loop, whose barriers make
  // them visible.  Rows past n get -1 and -2: they are no candidates anyway (col < n, row < n in gt_sym_argmax)
  __shared__ int s_group[2][GT_T];
  {
    const int side = tid >> 7, l = tid & (GT_T - 1);
    const int at = (side ? tj : ti) * GT_T + l;
    s_group[side][l] = at < n ? group[at] : -1 - side;
  }

  f32x4 acc[4][4];
  gt_tile(sums, ld, n, d, ti, tj, lds, acc, tid, wm, wn, fr, fq);

  // scores as in ahc_nearest_kernel: acc[i][j][r] · (inv[row] · inv[col]); the product of the two factors commutes
  const int rbase = ti * GT_T + wm * 64, cbase = tj * GT_T + wn * 64;
  float invc[4];
  int groupc[4], groupr[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = cbase + 16 * j + fr;
    invc[j] = col < n ? inv_count[col] : 0.f;
    groupc[j] = s_group[1][wn * 64 + 16 * j + fr];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rbase + 16 * i + 4 * fq + r;
      const float invr = row < n ? inv_count[row] : 0.f;
      groupr[i][r] = s_group[0][wm * 64 + 16 * i + 4 * fq + r];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j][r] *= invr * invc[j];
    }

  // only a pair inside ONE group is a candidate
  gt_sym_argmax(acc, [&](int i, int r, int j) { return groupr[i][r] == groupc[j]; }, ti, tj, slot_row, slot_col, n, npad, red_v, red_i,
                ws_val, ws_idx, tid, wm, wn, fr, fq);
}

// the slots of a row, and the two promises about `group`: it never decreases, and no group has more than max_group rows (group is
// monotone, so a larger group shows as group[i] == group[i + max_group]).  *bad was set to 0 before the launch; every thread that
// finds a broken promise stores the same 1
__global__ __launch_bounds__(256) void ahc_nearest_grouped_finish_kernel(const float* __restrict__ ws_val, const int* __restrict__ ws_idx,
                                                                         const int slots, const int npad, const int n,
                                                                         const int* __restrict__ group, const int max_group,
                                                                         int* __restrict__ nn, float* __restrict__ best,
                                                                         int* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) {
    const int g = group[i];
    const bool descends = i + 1 < n && group[i + 1] < g;
    const bool too_large = max_group < n - i && group[i + max_group] == g;
    if (descends || too_large) *bad = 1;
  }
  gt_finish(ws_val, ws_idx, slots, npad, n, nn, best, i);
}

}  // namespace

extern "C" size_t sd_ahc_nearest_grouped_workspace_bytes(int n, int d, int max_group) {
  return sd_rows_workspace_bytes(SD_ROWS_BAND, n, d, 1, GT_MAX_D, max_group);
}

extern "C" int sd_ahc_nearest_grouped_f32(const float* sums, long ld, int n, int d, const float* inv_count, const int* group, int max_group,
                                          int* nn, float* best, int* bad, void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const SdRowsCall c = {"sd_ahc_nearest_grouped_f32", "sums", SD_ROWS_BAND, n, d, ld, 1, GT_MAX_D, max_group};
  if (const int e = sd_rows_refused(c, sums, !(sums && inv_count && group && nn && best && bad && ws), ws, ws_bytes)) return e;
  const int nt = gt_tiles(n);
  const int band = ag_band(nt, max_group);      // W of the header
  const GtSymWs w = gt_sym_ws(ws, nt, 2 * band + 2);
  SD_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), stream));
  hipLaunchKernelGGL(ahc_nearest_grouped_kernel, dim3((unsigned)nt, (unsigned)(band + 1)), dim3(256), 0, stream, sums, ld, n, d, inv_count,
                     group, w.val, w.idx, w.npad, nt, band);
  SD_CHECK_LAUNCH("ahc_nearest_grouped_kernel");
  hipLaunchKernelGGL(ahc_nearest_grouped_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w.val, w.idx, w.slots, w.npad,
                     n, group, max_group, nn, best, bad);
  SD_CHECK_LAUNCH("ahc_nearest_grouped_finish_kernel");
  return SD_OK;
}
