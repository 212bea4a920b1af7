// HDBSCAN's two O(N^2) steps without the N x N matrix (include/sd_hip_hdbscan.h): the core value of every row (its k-th largest
// cosine to another row) and, per Boruvka round, the heaviest mutual-reachability edge that leaves the component of every row.
//
// Both kernels take their products from gt_tile() of sd_gram_tile.h, the tile of ahc_nearest_kernel (sd_ahc.hip): 128 x 128 per
// workgroup, acc[i][j][r] = <row rbase + 16 i + 4 fq + r, row cbase + 16 j + fr>, and <a, b> and <b, a> the same bits wherever they
// are computed.
//
// hdb_outgoing_kernel: ahc_nearest_kernel's walk (tiles on and above the diagonal), symmetric argmax, slots and finish (all of the
// header), with w = fminf(fminf(core[row], core[col]), acc) for the weight and comp[col] != comp[row] for the candidates.
//
// hdb_core_kernel<KK>: workgroup (c, I) walks the column tiles 8 c .. 8 c + 7 of row block I (full Gram).  After a tile's K loop the
// two waves of a column half put their accumulators into LDS (the staging buffer, reused: 128 rows x 64 columns, stride 65), and
// thread t scans 32 of them for row t % 128 into a sorted top-KK in registers (KK = k rounded up to 1, 2, 4, 8, 16; entries past the
// real ones are -inf).  The two threads of a row merge at the end; slot c of the row gets its k best.  hdb_core_finish_kernel merges
// the slots and writes the k-th.
#include <hip/hip_runtime.h>

#include <cmath>

#include "sd_common.h"
#include "hdbscan/sd_hdb_scan.h"
#include "sd_gram_tile.h"
#include "sd_hip_hdbscan.h"

namespace {

// HD_SC, hd_insert, the scan of a tile and the merges: hdbscan/sd_hdb_scan.h and the two body files beside it, shared with the grouped
// core pass (hdbscan/sd_hdb_grouped.hip)

// ----------------------------------------------------------------------------------------------------------------- core values

template <int KK>
__global__ __launch_bounds__(256, 2) void hdb_core_kernel(const float* __restrict__ rows, const long ld, const int n, const int d, const int k,
                                                          float* __restrict__ ws, const int npad, const int nt) {
  __shared__ __attribute__((aligned(16))) float lds[2 * GT_T * GT_LDS];
  const int ti = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int lrow = tid & (GT_T - 1), half = tid >> 7;        // the scan: 32 columns of a 64-column half-tile for row lrow
  const int row = ti * GT_T + lrow;

  float top[KK];
#pragma unroll
  for (int q = 0; q < KK; ++q) top[q] = -INFINITY;

  const int tj0 = blockIdx.x * HD_CHUNK;
  const int tj1 = tj0 + HD_CHUNK < nt ? tj0 + HD_CHUNK : nt;
  for (int tj = tj0; tj < tj1; ++tj) {
    f32x4 acc[4][4];
    gt_tile(rows, ld, n, d, ti, tj, lds, acc, tid, wm, wn, fr, fq);
#define HD_SCAN_CAND(col, at) ((col) != row)
#include "hdbscan/sd_hdb_scan_body.h"
#undef HD_SCAN_CAND
  }

#include "hdbscan/sd_hdb_halves_body.h"
}

template <int KK>
__global__ __launch_bounds__(256) void hdb_core_finish_kernel(const float* __restrict__ ws, const int chunks, const int npad, const int n,
                                                              const int k, float* __restrict__ core) {
  hd_finish<KK>(ws, chunks, npad, n, k, core, blockIdx.x * 256 + threadIdx.x);
}

// ----------------------------------------------------------------------------------------------------------------- outgoing edges

__global__ __launch_bounds__(256, 2) void hdb_outgoing_kernel(const float* __restrict__ rows, const long ld, const int n, const int d,
                                                              const float* __restrict__ core, const int* __restrict__ comp,
                                                              float* __restrict__ ws_val, int* __restrict__ ws_idx, const int npad) {
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

  // core and comp of the tile's 128 rows ([0]) and 128 columns ([1]): one coalesced load per thread, issued before the K loop, whose
  // barriers make them visible; the epilogue reads LDS and does not wait on memory
  __shared__ float s_core[2][GT_T];
  __shared__ int s_comp[2][GT_T];
  {
    const int side = tid >> 7, l = tid & (GT_T - 1);
    const int at = (side ? tj : ti) * GT_T + l;
    s_core[side][l] = at < n ? core[at] : 0.f;
    s_comp[side][l] = at < n ? comp[at] : 0;
  }

  f32x4 acc[4][4];
  gt_tile(rows, ld, n, d, ti, tj, lds, acc, tid, wm, wn, fr, fq);

  // w = fminf(fminf(core[row], core[col]), score): the inner fminf commutes, so the mirrored element is the same bits
  int compc[4], compr[4][4];
  float corec[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    corec[j] = s_core[1][wn * 64 + 16 * j + fr];
    compc[j] = s_comp[1][wn * 64 + 16 * j + fr];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float corer = s_core[0][wm * 64 + 16 * i + 4 * fq + r];
      compr[i][r] = s_comp[0][wm * 64 + 16 * i + 4 * fq + r];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j][r] = fminf(fminf(corer, corec[j]), acc[i][j][r]);
    }

  // only an edge into ANOTHER component is a candidate
  gt_sym_argmax(acc, [&](int i, int r, int j) { return compr[i][r] != compc[j]; }, ti, tj, tj + 1, ti, n, npad, red_v, red_i, ws_val, ws_idx,
                tid, wm, wn, fr, fq);
}

__global__ __launch_bounds__(256) void hdb_outgoing_finish_kernel(const float* __restrict__ ws_val, const int* __restrict__ ws_idx,
                                                                  const int slots, const int npad, const int n, int* __restrict__ nn,
                                                                  float* __restrict__ best) {
  gt_finish(ws_val, ws_idx, slots, npad, n, nn, best, blockIdx.x * 256 + threadIdx.x);
}

// the two launches of the core pass at KK = k rounded up to 1, 2, 4, 8, 16; the caller names the instantiation beside its number
template <int KK>
int hd_launch_core(const float* rows, long ld, int n, int d, int k, float* core, void* ws, hipStream_t stream, const char* core_label,
                   const char* finish_label) {
  const int nt = gt_tiles(n), npad = nt * GT_T, chunks = hd_chunks(nt);
  hipLaunchKernelGGL(hdb_core_kernel<KK>, dim3((unsigned)chunks, (unsigned)nt), dim3(256), 0, stream, rows, ld, n, d, k, static_cast<float*>(ws), npad, nt);
  SD_CHECK_LAUNCH(core_label);
  hipLaunchKernelGGL(hdb_core_finish_kernel<KK>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, static_cast<float*>(ws), chunks, npad, n, k, core);
  SD_CHECK_LAUNCH(finish_label);
  return SD_OK;
}

}  // namespace

extern "C" int sd_hdbscan_abi_version(void) { return SD_HDBSCAN_ABI_VERSION; }

extern "C" size_t sd_hdb_core_workspace_bytes(int n, int d, int k) { return sd_rows_workspace_bytes(SD_ROWS_CORE, n, d, 1, GT_MAX_D, k); }

extern "C" int sd_hdb_core_f32(const float* rows, long ld, int n, int d, int k, float* core, void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const SdRowsCall c = {"sd_hdb_core_f32", "rows", SD_ROWS_CORE, n, d, ld, 1, GT_MAX_D, k};
  if (const int e = sd_rows_refused(c, rows, !(rows && core && ws), ws, ws_bytes)) return e;
  if (k == 1) return hd_launch_core<1>(rows, ld, n, d, k, core, ws, stream, "hdb_core_kernel<1>", "hdb_core_finish_kernel<1>");
  if (k == 2) return hd_launch_core<2>(rows, ld, n, d, k, core, ws, stream, "hdb_core_kernel<2>", "hdb_core_finish_kernel<2>");
  if (k <= 4) return hd_launch_core<4>(rows, ld, n, d, k, core, ws, stream, "hdb_core_kernel<4>", "hdb_core_finish_kernel<4>");
  if (k <= 8) return hd_launch_core<8>(rows, ld, n, d, k, core, ws, stream, "hdb_core_kernel<8>", "hdb_core_finish_kernel<8>");
  return hd_launch_core<16>(rows, ld, n, d, k, core, ws, stream, "hdb_core_kernel<16>", "hdb_core_finish_kernel<16>");
}

extern "C" size_t sd_hdb_outgoing_workspace_bytes(int n, int d) { return sd_rows_workspace_bytes(SD_ROWS_SYM, n, d, 1, GT_MAX_D); }

extern "C" int sd_hdb_outgoing_f32(const float* rows, long ld, int n, int d, const float* core, const int* comp, int* nn, float* best,
                                   void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const SdRowsCall c = {"sd_hdb_outgoing_f32", "rows", SD_ROWS_SYM, n, d, ld, 1, GT_MAX_D};
  if (const int e = sd_rows_refused(c, rows, !(rows && core && comp && nn && best && ws), ws, ws_bytes)) return e;
  const int nt = gt_tiles(n);
  const GtSymWs w = gt_sym_ws(ws, nt, nt + 1);
  hipLaunchKernelGGL(hdb_outgoing_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, stream, rows, ld, n, d, core, comp, w.val, w.idx,
                     w.npad);
  SD_CHECK_LAUNCH("hdb_outgoing_kernel");
  hipLaunchKernelGGL(hdb_outgoing_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w.val, w.idx, w.slots, w.npad, n, nn,
                     best);
  SD_CHECK_LAUNCH("hdb_outgoing_finish_kernel");
  return SD_OK;
}
