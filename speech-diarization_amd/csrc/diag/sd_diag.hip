// Whitening statistics, the whitening transform and cluster centres in f64 (include/sd_hip_diag.h).  The two O(N d^2) products run on
// v_mfma_f64_16x16x4_f64; everything else is one thread per column or per element.  The sizes are launch bound (N of 50 to 50 000,
// d <= 256), so the structure is the simplest one whose summation order is fixed by the shape: partial results per block of
// SD_WHITEN_ROWS rows in a workspace, added in block order by a second kernel.  No floating-point atomics.
//
// Register layout of v_mfma_f64_16x16x4_f64 (lane l, fr = l & 15, fq = l >> 4): A holds A[row fr][k fq], B holds B[k fq][col fr], one
// f64 each; C/D register r holds D[row fq + 4 r][col fr].  This is NOT the f32 16x16x4 map (row 4 fq + r).
#include <hip/hip_runtime.h>

#include "sd_common.h"
#include "sd_hip_diag.h"
#include "sd_rows_check.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// DG_ROWS (SD_WHITEN_ROWS), DG_MAX_D (256), DG_MAX_K (1024), dg_tiles and dg_blocks: sd_rows_check.h, with the workspace they size
constexpr int DG_MAX_TILES = DG_MAX_D / 16;

// one thread per column: the rows of block blockIdx.x in ascending order -> part[block][16 T]; columns [d, 16 T) stay unwritten, unread
__global__ __launch_bounds__(256) void whiten_colsum_kernel(const float* __restrict__ x, const long ld, const int n, const int d,
                                                            double* __restrict__ part, const int dp) {
  const int c = threadIdx.x;
  if (c >= d) return;
  const int r0 = blockIdx.x * DG_ROWS;
  const int r1 = min(n, r0 + DG_ROWS);
  double s = 0.0;
  for (int r = r0; r < r1; ++r) s += (double)x[(size_t)r * ld + c];
  part[(size_t)blockIdx.x * dp + c] = s;
}

// one thread per column: the block sums in ascending order, divided by n
__global__ __launch_bounds__(256) void whiten_mean_kernel(const double* __restrict__ part, const int nb, const int dp, const int n, const int d,
                                                          double* __restrict__ mean) {
  const int c = threadIdx.x;
  if (c >= d) return;
  double s = 0.0;
  for (int b = 0; b < nb; ++b) s += part[(size_t)b * dp + c];
  mean[c] = s / (double)n;
}

// tile pair p of the upper triangle of T x T tiles, row by row: (0,0) (0,1) .. (0,T-1) (1,1) ..
__device__ __forceinline__ void dg_pair(int p, const int T, int& ti, int& tj) {
  ti = 0;
  while (p >= T - ti) {
    p -= T - ti;
    ++ti;
  }
  tj = ti + p;
}

// one wave per (row block, tile pair): D[a][b] += sum over the block's rows of xc[row][16 ti + a] xc[row][16 tj + b], four rows per MFMA
__global__ __launch_bounds__(64) void whiten_gram_kernel(const float* __restrict__ x, const long ld, const int n, const int d,
                                                         const double* __restrict__ mean, double* __restrict__ part, const int T) {
  const int lane = threadIdx.x;
  const int fr = lane & 15, fq = lane >> 4;
  int ti, tj;
  dg_pair(blockIdx.y, T, ti, tj);
  const int ca = 16 * ti + fr, cb = 16 * tj + fr;
  const bool oka = ca < d, okb = cb < d;
  const double ma = oka ? mean[ca] : 0.0, mb = okb ? mean[cb] : 0.0;
  const int r0 = blockIdx.x * DG_ROWS;
  const int rows = min(DG_ROWS, n - r0);
  f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < rows; s += 4) {
    const int row = r0 + s + fq;
    const bool okr = row < n;
    const float* const xr = x + (size_t)row * ld;
    const double a = okr && oka ? (double)xr[ca] - ma : 0.0;
    const double b = okr && okb ? (double)xr[cb] - mb : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  double* const out = part + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 256;
#pragma unroll
  for (int r = 0; r < 4; ++r) out[r * 64 + lane] = acc[r];
}

// one thread per element of tile pair blockIdx.x: the block partials in ascending order; on and above the diagonal, mirrored below
__global__ __launch_bounds__(256) void whiten_gram_finish_kernel(const double* __restrict__ part, const int nb, const int P, const int T,
                                                                 const int d, double* __restrict__ gram, const long ldg) {
  int ti, tj;
  dg_pair(blockIdx.x, T, ti, tj);
  const int t = threadIdx.x;
  const int lane = t & 63, reg = t >> 6;
  const int row = (lane >> 4) + 4 * reg, col = lane & 15;
  const int a = 16 * ti + row, b = 16 * tj + col;
  if (a >= d || b >= d || a > b) return;
  double s = 0.0;
  for (int k = 0; k < nb; ++k) s += part[((size_t)k * P + blockIdx.x) * 256 + t];
  gram[(size_t)a * ldg + b] = s;
  gram[(size_t)b * ldg + a] = s;
}

// one wave per 16 rows: v = (x - mean) W over every column tile, then the row norms and one rounding to f32
__global__ __launch_bounds__(64) void whiten_apply_kernel(const float* __restrict__ x, const long ld, const int n, const int d,
                                                          const double* __restrict__ mean, const double* __restrict__ w, const long ldw,
                                                          const double eps_add, float* __restrict__ out, const long ldo) {
  const int lane = threadIdx.x;
  const int fr = lane & 15, fq = lane >> 4;
  const int r0 = blockIdx.x * 16;
  const int arow = r0 + fr;
  const bool okr = arow < n;
  const float* const xr = x + (size_t)(okr ? arow : 0) * ld;
  f64x4 acc[DG_MAX_TILES];
#pragma unroll
  for (int j = 0; j < DG_MAX_TILES; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < d; k0 += 4) {
    const int kc = k0 + fq;
    const bool okk = kc < d;
    const double a = okr && okk ? (double)xr[kc] - mean[kc] : 0.0;
    const double* const wr = w + (size_t)(okk ? kc : 0) * ldw;
#pragma unroll
    for (int j = 0; j < DG_MAX_TILES; ++j) {
      if (16 * j < d) {                     // wave-uniform
        const int cb = 16 * j + fr;
        const double b = okk && cb < d ? wr[cb] : 0.0;
        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < DG_MAX_TILES; ++j) s += acc[j][r] * acc[j][r];      // columns past d hold zeros
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);             // a + b on both sides: every lane of the row gets the same bits
    const double den = sqrt(s) + eps_add;
    const int row = r0 + fq + 4 * r;
    if (row < n) {
      float* const orow = out + (size_t)row * ldo;
#pragma unroll
      for (int j = 0; j < DG_MAX_TILES; ++j) {
        const int col = 16 * j + fr;
        if (col < d) orow[col] = (float)(acc[j][r] / den);
      }
    }
  }
}

// one workgroup per label, one thread per column: the labels pass through LDS 256 at a time, rows are added in ascending order
__global__ __launch_bounds__(256) void label_centroids_kernel(const float* __restrict__ x, const long ld, const int n, const int d,
                                                              const int* __restrict__ labels, const double eps_add, float* __restrict__ out,
                                                              const long ldo, int* __restrict__ count) {
  __shared__ int lab[256];
  __shared__ double red[256];
  const int c = blockIdx.x;
  const int t = threadIdx.x;
  double s = 0.0;
  int cnt = 0;
  for (int base = 0; base < n; base += 256) {
    const int i = base + t;
    lab[t] = i < n ? labels[i] : -1;
    __syncthreads();
    if (t < d) {
      const int m = min(256, n - base);
      for (int j = 0; j < m; ++j)
        if (lab[j] == c) {
          s += (double)x[(size_t)(base + j) * ld + t];
          ++cnt;
        }
    }
    __syncthreads();
  }
  const double m = cnt ? s / (double)cnt : 0.0;
  red[t] = t < d ? m * m : 0.0;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) red[t] += red[t + o];
    __syncthreads();
  }
  const double den = sqrt(red[0]) + eps_add;
  if (t < d) out[(size_t)c * ldo + t] = cnt ? (float)(m / den) : 0.f;
  if (t == 0) count[c] = cnt;
}

}  // namespace

extern "C" int sd_diag_abi_version(void) { return SD_DIAG_ABI_VERSION; }

extern "C" size_t sd_whiten_stats_workspace_bytes(int n, int d) { return sd_rows_workspace_bytes(SD_ROWS_WHITEN, n, d, 2, DG_MAX_D); }

extern "C" int sd_whiten_stats_f64(const float* x, long ld, int n, int d, double* mean, double* gram, long ldg, void* ws, size_t ws_bytes,
                                   sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const SdRowsCall c = {"sd_whiten_stats_f64", "x", SD_ROWS_WHITEN, n, d, ld, 2, DG_MAX_D, 0, {{"ldg", ldg}}};
  if (const int e = sd_rows_refused(c, x, !(x && mean && gram && ws), ws, ws_bytes)) return e;
  const int T = dg_tiles(d), nb = dg_blocks(n), P = T * (T + 1) / 2, dp = 16 * T;
  double* const colsum = static_cast<double*>(ws);                 // [nb][dp]
  double* const tiles = colsum + (size_t)nb * dp;                  // [nb][P][256]
  hipLaunchKernelGGL(whiten_colsum_kernel, dim3((unsigned)nb), dim3(256), 0, stream, x, ld, n, d, colsum, dp);
  SD_CHECK_LAUNCH("whiten_colsum_kernel");
  hipLaunchKernelGGL(whiten_mean_kernel, dim3(1), dim3(256), 0, stream, colsum, nb, dp, n, d, mean);
  SD_CHECK_LAUNCH("whiten_mean_kernel");
  hipLaunchKernelGGL(whiten_gram_kernel, dim3((unsigned)nb, (unsigned)P), dim3(64), 0, stream, x, ld, n, d, mean, tiles, T);
  SD_CHECK_LAUNCH("whiten_gram_kernel");
  hipLaunchKernelGGL(whiten_gram_finish_kernel, dim3((unsigned)P), dim3(256), 0, stream, tiles, nb, P, T, d, gram, ldg);
  SD_CHECK_LAUNCH("whiten_gram_finish_kernel");
  return SD_OK;
}

extern "C" int sd_whiten_apply_f64(const float* x, long ld, int n, int d, const double* mean, const double* w, long ldw, double eps_add,
                                   float* out, long ldo, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const SdRowsCall c = {"sd_whiten_apply_f64", "x", SD_ROWS_ONLY, n, d, ld, 1, DG_MAX_D, 0, {{"ldw", ldw}, {"ldo", ldo}}};
  if (const int e = sd_rows_refused(c, x, !(x && mean && w && out))) return e;
  hipLaunchKernelGGL(whiten_apply_kernel, dim3((unsigned)((n + 15) / 16)), dim3(64), 0, stream, x, ld, n, d, mean, w, ldw, eps_add, out, ldo);
  SD_CHECK_LAUNCH("whiten_apply_kernel");
  return SD_OK;
}

extern "C" int sd_label_centroids_f32(const float* x, long ld, int n, int d, const int* labels, int k, double eps_add, float* out, long ldo,
                                      int* count, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  const SdRowsCall c = {"sd_label_centroids_f32", "x", SD_ROWS_LABELS, n, d, ld, 1, DG_MAX_D, k, {{"ldo", ldo}}};
  if (const int e = sd_rows_refused(c, x, !(x && labels && out && count))) return e;
  hipLaunchKernelGGL(label_centroids_kernel, dim3((unsigned)k), dim3(256), 0, stream, x, ld, n, d, labels, eps_add, out, ldo, count);
  SD_CHECK_LAUNCH("label_centroids_kernel");
  return SD_OK;
}
