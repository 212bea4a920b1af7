// HDBSCAN's two O(N^2) steps without the N x N matrix (include/sd_hip_hdbscan.h): the core value of every row (its k-th largest
// cosine to another row) and, per Boruvka round, the heaviest mutual-reachability edge that leaves the component of every row.
//
// The tile.  hd_tile() is a COPY of the K loop of ahc_nearest_kernel (sd_ahc.hip), not a shared header: sd_ahc.hip stays as it is,
// byte for byte.  A workgroup is 4 waves as 2 x 2 and owns one 128 x 128 tile; a wave owns 64 x 64 = 4 x 4 accumulators of
// v_mfma_f32_16x16x4_f32.  Operands: the 128 rows of the row block and of the column block, 32 k at a time, memory -> registers -> LDS
// (row stride 36 floats), the loads of the next 32 k issued before the MFMAs of the current ones.  A lane reads four consecutive k at
// chunk fq = lane / 16 and feeds element r to MFMA r; both operands use the same permutation and every tile of BOTH kernels walks k
// in the same order, so <a, b> and <b, a> are the same bits wherever they are computed.  Columns [d, ld) are not read.
//   acc[i][j][r] = <row rbase + 16 i + 4 fq + r, row cbase + 16 j + fr>.
//
// hdb_outgoing_kernel: ahc_nearest_kernel's walk (tiles on and above the diagonal), slots and finish, with w = fminf(fminf(core[row],
// core[col]), acc) in place of the scaled score and comp[col] != comp[row] in place of col != row.  The mirrored half reads the same w.
//
// hdb_core_kernel<KK>: workgroup (c, I) walks the column tiles 8 c .. 8 c + 7 of row block I (full Gram).  After a tile's K loop the
// two waves of a column half put their accumulators into LDS (the staging buffer, reused: 128 rows x 64 columns, stride 65), and
// thread t scans 32 of them for row t % 128 into a sorted top-KK in registers (KK = k rounded up to 1, 2, 4, 8, 16; entries past the
// real ones are -inf).  The two threads of a row merge at the end; slot c of the row gets its k best.  hdb_core_finish_kernel merges
// the slots and writes the k-th.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "sd_common.h"
#include "sd_hip_hdbscan.h"

namespace {

constexpr int HD_T = 128;                 // tile edge
constexpr int HD_KC = 32;                 // k of one staged chunk
constexpr int HD_LDS = HD_KC + 4;         // LDS row stride, floats: rows stay 16-byte aligned, consecutive rows shift by 4 banks
constexpr int HD_MAX_D = 1024;
constexpr int HD_MAX_TILES = 65535;       // grid.y
constexpr int HD_MAX_K = 16;
constexpr int HD_CHUNK = 8;               // column tiles per workgroup of the core pass
constexpr int HD_SC = 65;                 // row stride of the score half-tile in LDS: a wave's 64 rows fall into distinct banks
static_assert(HD_T * HD_SC <= 2 * HD_T * HD_LDS, "the score half-tile reuses the staging buffer");
static_assert(HD_T * (HD_MAX_K + 1) <= 2 * HD_T * HD_LDS, "so does the merge of the two threads of a row");

// columns c .. c + 3 of a row (c % 4 == 0), zeros from column d on; nothing at or past d is read
__device__ __forceinline__ f32x4 hd_load4(const float* __restrict__ row, int c, int d) {
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
__device__ __forceinline__ void hd_take(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// the component mask of the outgoing pass: only an edge into ANOTHER component is a candidate
__device__ __forceinline__ bool hd_leaves(int comp_a, int comp_b) { return comp_a != comp_b; }

// acc <- the products of tile (ti, tj); `lds` holds 2 * HD_T * HD_LDS floats.  Starts with a barrier before it touches LDS; the caller
// puts one after it before LDS is reused.
__device__ __forceinline__ void hd_tile(const float* __restrict__ rows, const long ld, const int n, const int d, const int ti, const int tj,
                                        float* __restrict__ lds, f32x4 (&acc)[4][4]) {
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
    int m = ti * HD_T + r0 + 32 * i;
    int c = tj * HD_T + r0 + 32 * i;
    m = m < n ? m : n - 1;                  // rows past n read row n - 1; their scores are never taken
    c = c < n ? c : n - 1;
    pa[i] = rows + (size_t)m * ld;
    pb[i] = rows + (size_t)c * ld;
  }
  f32x4 ra[4], rb[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = hd_load4(pa[i], k0 + 4 * g, d);
      rb[i] = hd_load4(pb[i], k0 + 4 * g, d);
    }
  };

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float* const a_base = lds + (wm * 64 + fr) * HD_LDS;
  const float* const b_base = lds + (HD_T + wn * 64 + fr) * HD_LDS;
  const int nk = (d + HD_KC - 1) / HD_KC;
  fetch(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                        // every wave is done with the previous chunk
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<f32x4*>(&lds[(r0 + 32 * i) * HD_LDS + 4 * g]) = ra[i];
      *reinterpret_cast<f32x4*>(&lds[(HD_T + r0 + 32 * i) * HD_LDS + 4 * g]) = rb[i];
    }
    __syncthreads();
    if (kt + 1 < nk) fetch((kt + 1) * HD_KC);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int off = 16 * h + 4 * fq;
      f32x4 av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const f32x4*>(a_base + i * 16 * HD_LDS + off);
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const f32x4*>(b_base + j * 16 * HD_LDS + off);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][r], bv[j][r], acc[i][j], 0, 0, 0);
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------- core values

// v into the descending list top[0 .. KK): equal values are kept as often as they come (a multiset)
template <int KK>
__device__ __forceinline__ void hd_insert(float (&top)[KK], float v) {
  if (v > top[KK - 1]) {
#pragma unroll
    for (int q = 0; q < KK; ++q) {
      if (v > top[q]) {
        const float t = top[q];
        top[q] = v;
        v = t;
      }
    }
  }
}

template <int KK>
__global__ __launch_bounds__(256, 2) void hdb_core_kernel(const float* __restrict__ rows, const long ld, const int n, const int d, const int k,
                                                          float* __restrict__ ws, const int npad, const int nt) {
  __shared__ __attribute__((aligned(16))) float lds[2 * HD_T * HD_LDS];
  const int ti = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int lrow = tid & (HD_T - 1), half = tid >> 7;        // the scan: 32 columns of a 64-column half-tile for row lrow
  const int row = ti * HD_T + lrow;

  float top[KK];
#pragma unroll
  for (int q = 0; q < KK; ++q) top[q] = -INFINITY;

  const int tj0 = blockIdx.x * HD_CHUNK;
  const int tj1 = tj0 + HD_CHUNK < nt ? tj0 + HD_CHUNK : nt;
  for (int tj = tj0; tj < tj1; ++tj) {
    f32x4 acc[4][4];
    hd_tile(rows, ld, n, d, ti, tj, lds, acc);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      __syncthreads();                      // the operands (h = 0) or the previous half (h = 1) have been read
      if (wn == h) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) lds[(wm * 64 + 16 * i + 4 * fq + r) * HD_SC + 16 * j + fr] = acc[i][j][r];
      }
      __syncthreads();
      const int c0 = half * 32;
      const int col0 = tj * HD_T + h * 64 + c0;
      const float* const src = lds + lrow * HD_SC + c0;
      for (int c = 0; c < 32; ++c) {
        const int col = col0 + c;
        if (col < n && col != row) hd_insert<KK>(top, src[c]);
      }
    }
  }

  // the two threads of a row: the upper one hands its list over, the lower one merges and writes the k best of this chunk
  __syncthreads();
  if (half == 1) {
#pragma unroll
    for (int q = 0; q < KK; ++q) lds[lrow * (KK + 1) + q] = top[q];
  }
  __syncthreads();
  if (half == 0) {
#pragma unroll
    for (int q = 0; q < KK; ++q) hd_insert<KK>(top, lds[lrow * (KK + 1) + q]);
    float* const out = ws + (size_t)blockIdx.x * k * npad + row;       // slot [chunk][q][padded row]
#pragma unroll
    for (int q = 0; q < KK; ++q)
      if (q < k) out[(size_t)q * npad] = top[q];
  }
}

template <int KK>
__global__ __launch_bounds__(256) void hdb_core_finish_kernel(const float* __restrict__ ws, const int chunks, const int npad, const int n,
                                                              const int k, float* __restrict__ core) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float top[KK];
#pragma unroll
  for (int q = 0; q < KK; ++q) top[q] = -INFINITY;
  for (int s = 0; s < chunks * k; ++s) hd_insert<KK>(top, ws[(size_t)s * npad + i]);
  float out = top[0];
#pragma unroll
  for (int q = 1; q < KK; ++q)
    if (q == k - 1) out = top[q];
  core[i] = out;
}

// ----------------------------------------------------------------------------------------------------------------- outgoing edges

__global__ __launch_bounds__(256, 2) void hdb_outgoing_kernel(const float* __restrict__ rows, const long ld, const int n, const int d,
                                                              const float* __restrict__ core, const int* __restrict__ comp,
                                                              float* __restrict__ ws_val, int* __restrict__ ws_idx, const int npad) {
  const int tj = blockIdx.x, ti = blockIdx.y;
  if (ti > tj) return;                      // workgroup-uniform: below the diagonal
  __shared__ __attribute__((aligned(16))) float lds[2 * HD_T * HD_LDS];
  __shared__ float red_v[2][HD_T];
  __shared__ int red_i[2][HD_T];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int fr = lane & 15, fq = lane >> 4;

  // core and comp of the tile's 128 rows ([0]) and 128 columns ([1]): one coalesced load per thread, issued before the K loop, whose
  // barriers make them visible; the epilogue reads LDS and does not wait on memory
  __shared__ float s_core[2][HD_T];
  __shared__ int s_comp[2][HD_T];
  {
    const int side = tid >> 7, l = tid & (HD_T - 1);
    const int at = (side ? tj : ti) * HD_T + l;
    s_core[side][l] = at < n ? core[at] : 0.f;
    s_comp[side][l] = at < n ? comp[at] : 0;
  }

  f32x4 acc[4][4];
  hd_tile(rows, ld, n, d, ti, tj, lds, acc);

  // w = fminf(fminf(core[row], core[col]), score): the inner fminf commutes, so the mirrored element is the same bits
  const int rbase = ti * HD_T + wm * 64, cbase = tj * HD_T + wn * 64;
  const bool diag = ti == tj;
  int col[4], compc[4], compr[4][4];
  float corec[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    col[j] = cbase + 16 * j + fr;
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

  // row maxima over the tile's columns in another component -> slot tj + 1 of row block ti
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rbase + 16 * i + 4 * fq + r;
      float bv = -INFINITY;
      int bi = INT_MAX;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (col[j] < n && hd_leaves(compr[i][r], compc[j]) && (!diag || col[j] > row)) hd_take(bv, bi, acc[i][j][r], col[j]);
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        hd_take(bv, bi, ov, oi);
      }
      if (fr == 0) {
        red_v[wn][wm * 64 + 16 * i + 4 * fq + r] = bv;
        red_i[wn][wm * 64 + 16 * i + 4 * fq + r] = bi;
      }
    }
  __syncthreads();
  if (tid < HD_T) {
    float bv = red_v[0][tid];
    int bi = red_i[0][tid];
    hd_take(bv, bi, red_v[1][tid], red_i[1][tid]);
    const size_t at = (size_t)(tj + 1) * npad + (size_t)ti * HD_T + tid;
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
        if (row < n && hd_leaves(compr[i][r], compc[j]) && (!diag || row < col[j])) hd_take(bv, bi, acc[i][j][r], row);
      }
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      hd_take(bv, bi, ov, oi);
    }
    if (fq == 0) {
      red_v[wm][wn * 64 + 16 * j + fr] = bv;
      red_i[wm][wn * 64 + 16 * j + fr] = bi;
    }
  }
  __syncthreads();
  if (tid < HD_T) {
    float bv = red_v[0][tid];
    int bi = red_i[0][tid];
    hd_take(bv, bi, red_v[1][tid], red_i[1][tid]);
    const size_t at = (size_t)ti * npad + (size_t)tj * HD_T + tid;
    ws_val[at] = bv;
    ws_idx[at] = bi == INT_MAX ? -1 : bi;
  }
}

// the slots of row i in ascending column order, strict >: the lowest index among equal maxima
__global__ __launch_bounds__(256) void hdb_outgoing_finish_kernel(const float* __restrict__ ws_val, const int* __restrict__ ws_idx,
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

inline int hd_tiles(int n) { return (n + HD_T - 1) / HD_T; }
inline int hd_chunks(int nt) { return (nt + HD_CHUNK - 1) / HD_CHUNK; }

template <int KK>
int hd_launch_core(const float* rows, long ld, int n, int d, int k, float* core, float* ws, int nt, hipStream_t stream) {
  const int npad = nt * HD_T;
  const int chunks = hd_chunks(nt);
  hipLaunchKernelGGL(hdb_core_kernel<KK>, dim3((unsigned)chunks, (unsigned)nt), dim3(256), 0, stream, rows, ld, n, d, k, ws, npad, nt);
  SD_CHECK_LAUNCH(KK == 1 ? "hdb_core_kernel<1>" : KK == 2 ? "hdb_core_kernel<2>" : KK == 4 ? "hdb_core_kernel<4>" : KK == 8 ? "hdb_core_kernel<8>" : "hdb_core_kernel<16>");
  hipLaunchKernelGGL(hdb_core_finish_kernel<KK>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws, chunks, npad, n, k, core);
  SD_CHECK_LAUNCH(KK == 1 ? "hdb_core_finish_kernel<1>" : KK == 2 ? "hdb_core_finish_kernel<2>" : KK == 4 ? "hdb_core_finish_kernel<4>"
                  : KK == 8 ? "hdb_core_finish_kernel<8>" : "hdb_core_finish_kernel<16>");
  return SD_OK;
}

}  // namespace

extern "C" int sd_hdbscan_abi_version(void) { return SD_HDBSCAN_ABI_VERSION; }

extern "C" size_t sd_hdb_core_workspace_bytes(int n, int d, int k) {
  if (n <= 1 || d <= 0 || d > HD_MAX_D || k <= 0 || k > HD_MAX_K || k > n - 1) return 0;
  const size_t nt = (size_t)hd_tiles(n);
  return (size_t)hd_chunks((int)nt) * nt * HD_T * (size_t)k * sizeof(float);
}

extern "C" int sd_hdb_core_f32(const float* rows, long ld, int n, int d, int k, float* core, void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SD_CHECK_ARG(n > 0 && d > 0 && ld >= d, "sd_hdb_core_f32: n=%d d=%d ld=%ld", n, d, ld);
  if (d > HD_MAX_D) return sd_set_error(SD_ERR_UNSUPPORTED, "sd_hdb_core_f32: d=%d, at most %d columns are supported", d, HD_MAX_D);
  if (k > HD_MAX_K) return sd_set_error(SD_ERR_UNSUPPORTED, "sd_hdb_core_f32: k=%d, at most %d neighbours are supported", k, HD_MAX_K);
  SD_CHECK_ARG(k >= 1 && k <= n - 1, "sd_hdb_core_f32: k=%d must lie in 1 .. n - 1 (n=%d)", k, n);
  SD_CHECK_ARG(rows && core && ws, "sd_hdb_core_f32: null pointer");
  SD_CHECK_ARG(sd_aligned16(rows) && ld % 4 == 0, "sd_hdb_core_f32: rows must be 16-byte aligned with ld %% 4 == 0 (ld=%ld)", ld);
  SD_CHECK_ARG(sd_aligned16(ws), "sd_hdb_core_f32: workspace is not 16-byte aligned");
  const int nt = hd_tiles(n);
  if (nt > HD_MAX_TILES) return sd_set_error(SD_ERR_UNSUPPORTED, "sd_hdb_core_f32: n=%d, at most %d rows are supported", n, HD_MAX_TILES * HD_T);
  const size_t need = sd_hdb_core_workspace_bytes(n, d, k);
  if (ws_bytes < need)
    return sd_set_error(SD_ERR_WORKSPACE, "sd_hdb_core_f32: workspace of %zu bytes, n=%d d=%d k=%d needs %zu", ws_bytes, n, d, k, need);
  float* w = static_cast<float*>(ws);
  if (k == 1) return hd_launch_core<1>(rows, ld, n, d, k, core, w, nt, stream);
  if (k == 2) return hd_launch_core<2>(rows, ld, n, d, k, core, w, nt, stream);
  if (k <= 4) return hd_launch_core<4>(rows, ld, n, d, k, core, w, nt, stream);
  if (k <= 8) return hd_launch_core<8>(rows, ld, n, d, k, core, w, nt, stream);
  return hd_launch_core<16>(rows, ld, n, d, k, core, w, nt, stream);
}

extern "C" size_t sd_hdb_outgoing_workspace_bytes(int n, int d) {
  if (n <= 0 || d <= 0 || d > HD_MAX_D) return 0;
  const size_t nt = (size_t)hd_tiles(n);
  return (nt + 1) * nt * HD_T * (sizeof(float) + sizeof(int));
}

extern "C" int sd_hdb_outgoing_f32(const float* rows, long ld, int n, int d, const float* core, const int* comp, int* nn, float* best,
                                   void* ws, size_t ws_bytes, sd_stream_t stream_) {
  hipStream_t stream = static_cast<hipStream_t>(stream_);
  SD_CHECK_ARG(n > 0 && d > 0 && ld >= d, "sd_hdb_outgoing_f32: n=%d d=%d ld=%ld", n, d, ld);
  if (d > HD_MAX_D) return sd_set_error(SD_ERR_UNSUPPORTED, "sd_hdb_outgoing_f32: d=%d, at most %d columns are supported", d, HD_MAX_D);
  SD_CHECK_ARG(rows && core && comp && nn && best && ws, "sd_hdb_outgoing_f32: null pointer");
  SD_CHECK_ARG(sd_aligned16(rows) && ld % 4 == 0, "sd_hdb_outgoing_f32: rows must be 16-byte aligned with ld %% 4 == 0 (ld=%ld)", ld);
  SD_CHECK_ARG(sd_aligned16(ws), "sd_hdb_outgoing_f32: workspace is not 16-byte aligned");
  const int nt = hd_tiles(n);
  if (nt > HD_MAX_TILES)
    return sd_set_error(SD_ERR_UNSUPPORTED, "sd_hdb_outgoing_f32: n=%d, at most %d rows are supported", n, HD_MAX_TILES * HD_T);
  const size_t need = sd_hdb_outgoing_workspace_bytes(n, d);
  if (ws_bytes < need)
    return sd_set_error(SD_ERR_WORKSPACE, "sd_hdb_outgoing_f32: workspace of %zu bytes, n=%d d=%d needs %zu", ws_bytes, n, d, need);
  const int npad = nt * HD_T;
  const int slots = nt + 1;
  float* ws_val = static_cast<float*>(ws);
  int* ws_idx = reinterpret_cast<int*>(ws_val + (size_t)slots * npad);
  hipLaunchKernelGGL(hdb_outgoing_kernel, dim3((unsigned)nt, (unsigned)nt), dim3(256), 0, stream, rows, ld, n, d, core, comp, ws_val, ws_idx,
                     npad);
  SD_CHECK_LAUNCH("hdb_outgoing_kernel");
  hipLaunchKernelGGL(hdb_outgoing_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ws_val, ws_idx, slots, npad, n, nn,
                     best);
  SD_CHECK_LAUNCH("hdb_outgoing_finish_kernel");
  return SD_OK;
}
