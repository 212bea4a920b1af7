// HDBSCAN's two O(N^2) steps for MANY recordings at once (include/sd_hip_hdbscan.h, sd_hdb_core_grouped_f32 and
// sd_hdb_outgoing_grouped_f32): the rows of all recordings stand one after another, `group` names the recording of every row
// (non-decreasing), and a row's core value and every tree edge look only inside the row's own recording.  The tile, the symmetric
// argmax and the walk of the slots are sd_gram_tile.h's, the top-k scan is hdbscan/sd_hdb_scan.h's (that of hdb_core_kernel), the weight
// is hdb_outgoing_kernel's (sd_hdbscan.hip): a recording's scores are the bits it gets when it is clustered alone.
//
// Rows of one group lie at most max_group - 1 apart, so only the column tiles I - W .. I + W of row block I can hold a row of one of
// its groups: W = ag_band(T, max_group) = min(T - 1, ceil((max_group - 1) / 128)), T = ceil(n / 128).
//
// hdb_core_grouped_kernel<KK>: the walk of hdb_core_kernel over that band of the FULL Gram.  Grid (ceil((2 W + 1) / 8), T): workgroup
// (c, I) walks the column tiles I - W + 8 c .. I - W + 8 c + 7 (at most I + W).  A tile outside [0, T), or one whose column block
// shares no group with the row block (two loads of `group`, which is non-decreasing), is skipped workgroup-uniformly.  The scan takes
// a column only when group[col] == group[row].  Slot c of the row gets the k best of the chunk (-inf where there are fewer);
// hdb_core_grouped_finish_kernel<KK> merges the slots, writes the k-th and checks the two promises about `group`.
//
// hdb_outgoing_grouped_kernel: the walk, the empty-tile ownership and the 2 W + 2 slots of ahc_nearest_grouped_kernel
// (ahc/sd_ahc_grouped.hip, whose header describes them) with w = fminf(fminf(core[row], core[col]), acc) for the weight and
// group[col] == group[row] && comp[col] != comp[row] for the candidates.
//
// No index depends on the contents of `group`: a broken promise is reported through `bad` and can send no load or store out of bounds.
#include <hip/hip_runtime.h>

#include "sd_common.h"
#include "hdbscan/sd_hdb_scan.h"
#include "sd_gram_tile.h"
#include "sd_hip_hdbscan.h"

namespace {

// the two promises about `group` at row i < n: it never decreases, and no group has more than max_group rows (group is monotone, so a
// larger group shows as group[i] == group[i + max_group]).  *bad was set to 0 before the launch; every thread that finds a broken
// promise stores the same 1
__device__ __forceinline__ void hg_check_promises(const int* __restrict__ group, const int max_group, const int n, const int i,
                                                  int* __restrict__ bad) {
  const int g = group[i];
  const bool descends = i + 1 < n && group[i + 1] < g;
  const bool too_large = max_group < n - i && group[i + max_group] == g;
  if (descends || too_large) *bad = 1;
}

// ----------------------------------------------------------------------------------------------------------------- core values

template <int KK>
__global__ __launch_bounds__(256, 2) void hdb_core_grouped_kernel(const float* __restrict__ rows, const long ld, const int n, const int d,
                                                                  const int k, const int* __restrict__ group, float* __restrict__ ws,
                                                                  const int npad, const int nt, const int band) {
  __shared__ __attribute__((aligned(16))) float lds[2 * GT_T * GT_LDS];
  __shared__ int s_group[GT_T];             // the groups of the tile's 128 columns
  const int ti = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int lrow = tid & (GT_T - 1), half = tid >> 7;        // the scan: 32 columns of a 64-column half-tile for row lrow
  const int row = ti * GT_T + lrow;
  const int grow = row < n ? group[row] : -1;                 // rows past n: their slots are written and never read

  float top[KK];
#pragma unroll
  for (int q = 0; q < KK; ++q) top[q] = -INFINITY;

  const int tj0 = ti - band + (int)blockIdx.x * HD_CHUNK;
  const int tj1 = tj0 + HD_CHUNK < ti + band + 1 ? tj0 + HD_CHUNK : ti + band + 1;
  for (int tj = tj0; tj < tj1; ++tj) {
    // workgroup-uniform: a tile outside the matrix, or a row block and a column block that share no group (group is non-decreasing:
    // of two blocks, the largest group of the earlier one is that of its last row, the smallest of the later one that of its first).
    // ti, tj < nt and ti != tj: the earlier block is a full one, every index lies below n
    if (tj < 0 || tj >= nt) continue;
    if (tj < ti && group[tj * GT_T + GT_T - 1] != group[ti * GT_T]) continue;
    if (tj > ti && group[ti * GT_T + GT_T - 1] != group[tj * GT_T]) continue;
    __syncthreads();                        // the scan of the previous tile has read s_group
    if (tid < GT_T) {
      const int at = tj * GT_T + tid;
      s_group[tid] = at < n ? group[at] : -2;
    }
    f32x4 acc[4][4];
    gt_tile(rows, ld, n, d, ti, tj, lds, acc, tid, wm, wn, fr, fq);         // its barriers make s_group visible
#define HD_SCAN_CAND(col, at) ((col) != row && s_group[at] == grow)
#include "hdbscan/sd_hdb_scan_body.h"
#undef HD_SCAN_CAND
  }

#include "hdbscan/sd_hdb_halves_body.h"
}

template <int KK>
__global__ __launch_bounds__(256) void hdb_core_grouped_finish_kernel(const float* __restrict__ ws, const int chunks, const int npad,
                                                                      const int n, const int k, const int* __restrict__ group,
                                                                      const int max_group, float* __restrict__ core, int* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) hg_check_promises(group, max_group, n, i, bad);
  hd_finish<KK>(ws, chunks, npad, n, k, core, i);
}

// ----------------------------------------------------------------------------------------------------------------- outgoing edges

__global__ __launch_bounds__(256, 2) void hdb_outgoing_grouped_kernel(const float* __restrict__ rows, const long ld, const int n, const int d,
                                                                      const float* __restrict__ core, const int* __restrict__ comp,
                                                                      const int* __restrict__ group, float* __restrict__ ws_val,
                                                                      int* __restrict__ ws_idx, const int npad, const int nt, const int band) {
  const int ti = blockIdx.x, k = blockIdx.y;
  const int slot_row = band + 1 + k, slot_col = band - k;
  const int tid = threadIdx.x;
  int tj = ti + k;
  // workgroup-uniform: a tile past the last one (this workgroup then owns the empty left slot [band - k] of row block ti + k - T), or
  // a row block and a column block that share no group
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

  // core, comp and group of the tile's 128 rows ([0]) and 128 columns ([1]): one coalesced load each per thread, issued before the K
  // loop, whose barriers make them visible.  Rows past n get the groups -1 and -2: they are no candidates anyway
  __shared__ float s_core[2][GT_T];
  __shared__ int s_comp[2][GT_T];
  __shared__ int s_group[2][GT_T];
  {
    const int side = tid >> 7, l = tid & (GT_T - 1);
    const int at = (side ? tj : ti) * GT_T + l;
    s_core[side][l] = at < n ? core[at] : 0.f;
    s_comp[side][l] = at < n ? comp[at] : 0;
    s_group[side][l] = at < n ? group[at] : -1 - side;
  }

  f32x4 acc[4][4];
  gt_tile(rows, ld, n, d, ti, tj, lds, acc, tid, wm, wn, fr, fq);

  // w = fminf(fminf(core[row], core[col]), score), as in hdb_outgoing_kernel: the inner fminf commutes, so the mirrored element is the
  // same bits
  int compc[4], groupc[4], compr[4][4], groupr[4][4];
  float corec[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    corec[j] = s_core[1][wn * 64 + 16 * j + fr];
    compc[j] = s_comp[1][wn * 64 + 16 * j + fr];
    groupc[j] = s_group[1][wn * 64 + 16 * j + fr];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float corer = s_core[0][wm * 64 + 16 * i + 4 * fq + r];
      compr[i][r] = s_comp[0][wm * 64 + 16 * i + 4 * fq + r];
      groupr[i][r] = s_group[0][wm * 64 + 16 * i + 4 * fq + r];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j][r] = fminf(fminf(corer, corec[j]), acc[i][j][r]);
    }

  // only an edge into ANOTHER component of the SAME group is a candidate
  gt_sym_argmax(acc, [&](int i, int r, int j) { return groupr[i][r] == groupc[j] && compr[i][r] != compc[j]; }, ti, tj, slot_row, slot_col, n,
                npad, red_v, red_i, ws_val, ws_idx, tid, wm, wn, fr, fq);
}

__global__ __launch_bounds__(256) void hdb_outgoing_grouped_finish_kernel(const float* __restrict__ ws_val, const int* __restrict__ ws_idx,
                                                                          const int slots, const int npad, const int n,
                                                                          const int* __restrict__ group, const int max_group,
                                                                          int* __restrict__ nn, float* __restrict__ best,
                                                                          int* __restrict__ bad) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) hg_check_promises(group, max_group, n, i, bad);
  gt_finish(ws_val, ws_idx, slots, npad, n, nn, best, i);
}

// the two launches of the grouped core pass at KK = k rounded up to 1, 2, 4, 8, 16; the caller names the instantiation beside its number
template <int KK>
int hg_launch_core(const float* rows, long ld, int n, int d, int k, const int* group, int max_group, float* core, int* bad, void* ws,
                   hipStream_t stream, const char* core_label, const char* finish_label) {
  const int nt = gt_tiles(n), npad = nt * GT_T;
  const int band = ag_band(nt, max_group);      // W of the header
  const int chunks = hd_band_chunks(band);
  hipLaunchKernelGGL(hdb_core_grouped_kernel<KK>, dim3((unsigned)chunks, (unsigned)nt), dim3(256), 0, stream, rows, ld, n, d, k, group,
                     static_cast<float*>(ws), npad, nt, band);
  SD_CHECK_LAUNCH(core_label);
  hipLaunchKernelGGL(hdb_core_grouped_finish_kernel<KK>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, static_cast<float*>(ws), chunks,
                     npad, n, k, group, max_group, core, bad);
  SD_CHECK_LAUNCH(finish_label);
  return SD_OK;
}

}  // namespace

extern "C" size_t sd_hdb_core_grouped_workspace_bytes(int n, int d, int k, int max_group) {
  return sd_rows_workspace_bytes(SD_ROWS_BAND_CORE, n, d, 1, GT_MAX_D, k, max_group);
}

extern "C" int sd_hdb_core_grouped_f32(const float* rows, long ld, int n, int d, int k, const int* group, int max_group, float* core, int* bad,
                                       void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SdRowsCall c = {"sd_hdb_core_grouped_f32", "rows", SD_ROWS_BAND_CORE, n, d, ld, 1, GT_MAX_D, k};
  c.max_group = max_group;
  if (const int e = sd_rows_refused(c, rows, !(rows && group && core && bad && ws), ws, ws_bytes)) return e;
  SD_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), stream));
  if (k == 1) return hg_launch_core<1>(rows, ld, n, d, k, group, max_group, core, bad, ws, stream, "hdb_core_grouped_kernel<1>", "hdb_core_grouped_finish_kernel<1>");
  if (k == 2) return hg_launch_core<2>(rows, ld, n, d, k, group, max_group, core, bad, ws, stream, "hdb_core_grouped_kernel<2>", "hdb_core_grouped_finish_kernel<2>");
  if (k <= 4) return hg_launch_core<4>(rows, ld, n, d, k, group, max_group, core, bad, ws, stream, "hdb_core_grouped_kernel<4>", "hdb_core_grouped_finish_kernel<4>");
  if (k <= 8) return hg_launch_core<8>(rows, ld, n, d, k, group, max_group, core, bad, ws, stream, "hdb_core_grouped_kernel<8>", "hdb_core_grouped_finish_kernel<8>");
  return hg_launch_core<16>(rows, ld, n, d, k, group, max_group, core, bad, ws, stream, "hdb_core_grouped_kernel<16>", "hdb_core_grouped_finish_kernel<16>");
}

extern "C" size_t sd_hdb_outgoing_grouped_workspace_bytes(int n, int d, int max_group) {
  return sd_rows_workspace_bytes(SD_ROWS_BAND, n, d, 1, GT_MAX_D, max_group);
}

extern "C" int sd_hdb_outgoing_grouped_f32(const float* rows, long ld, int n, int d, const float* core, const int* comp, const int* group,
                                           int max_group, int* nn, float* best, int* bad, void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const SdRowsCall c = {"sd_hdb_outgoing_grouped_f32", "rows", SD_ROWS_BAND, n, d, ld, 1, GT_MAX_D, max_group};
  if (const int e = sd_rows_refused(c, rows, !(rows && core && comp && group && nn && best && bad && ws), ws, ws_bytes)) return e;
  const int nt = gt_tiles(n);
  const int band = ag_band(nt, max_group);
  const GtSymWs w = gt_sym_ws(ws, nt, 2 * band + 2);
  SD_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), stream));
  hipLaunchKernelGGL(hdb_outgoing_grouped_kernel, dim3((unsigned)nt, (unsigned)(band + 1)), dim3(256), 0, stream, rows, ld, n, d, core, comp,
                     group, w.val, w.idx, w.npad, nt, band);
  SD_CHECK_LAUNCH("hdb_outgoing_grouped_kernel");
  hipLaunchKernelGGL(hdb_outgoing_grouped_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w.val, w.idx, w.slots, w.npad,
                     n, group, max_group, nn, best, bad);
  SD_CHECK_LAUNCH("hdb_outgoing_grouped_finish_kernel");
  return SD_OK;
}
