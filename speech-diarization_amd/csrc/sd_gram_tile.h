// One 128 x 128 tile of the Gram matrix of f32 rows, its symmetric argmax and the walk of the argmax slots: the only statement of what
// sd_ahc.hip (ahc_nearest_kernel) and sd_hdbscan.hip (hdb_outgoing_kernel, hdb_core_kernel) compute with, so that <a, b> and <b, a>
// are the same bits wherever they are computed.  Device functions and host helpers only; the kernels stay in their files.
//
// A workgroup is 4 waves as 2 x 2 (wm = wave / 2 the row half, wn = wave % 2 the column half) and owns one tile; a wave owns
// 64 x 64 = 4 x 4 accumulators of v_mfma_f32_16x16x4_f32 (the arithmetic and the accumulator layout of the exact form of
// sd_affinity.hip), fr = lane % 16, fq = lane / 16.
// * Operands: the 128 rows of the tile's row block and of its column block, 32 k at a time, memory -> registers -> LDS (row stride
//   36 floats); the loads of the next 32 k are issued before the MFMAs of the current ones.  A lane reads four consecutive k
//   (ds_read_b128) at chunk fq and feeds element r to MFMA r, which sums k in {4 fq + r}; both operands use the same permutation
//   and every tile walks k in the same order.  Columns [d, ld) are not read: the last group of four is loaded element by element,
//   zeros past d.  acc[i][j][r] = <row rbase + 16 i + 4 fq + r, row cbase + 16 j + fr>, rbase = 128 ti + 64 wm, cbase = 128 tj + 64 wn.
// * Symmetric argmax, from registers, of the weights the caller has made of acc (a weight and its mirror must be the same bits)
//   for a tile on or above the diagonal.  Row maxima: over j in the lane, over fr across the 16-lane row, over the two waves of a
//   row through LDS -> slot [slot_row] of row block ti.  Column maxima (the row maxima of the mirrored tile, from the same
//   accumulators): over i, r in the lane, over fq across lanes 16 / 32 apart, over the two waves of a column -> slot [slot_col] of
//   row block tj.  The diagonal tile keeps col > row for the first and row < col for the second.  Among equal weights the lowest
//   index wins at every step.  The caller numbers the slots so that the columns a slot stands for ascend with it: the full walk
//   (sd_ahc.hip, sd_hdbscan.hip) passes tj + 1 and ti, the banded walk (ahc/sd_ahc_grouped.hip) its own.
// * gt_finish walks the slots of a row in ascending order with a strict >.
// * Every function takes the lane coordinates (tid, wm, wn, fr, fq) from the kernel.  Deriving them from threadIdx.x in here costs
//   ahc_nearest_kernel about 20 VGPRs and with them its third workgroup per CU.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "sd_common.h"
#include "sd_rows_check.h"

// GT_T (the tile edge, 128), GT_MAX_D, GT_MAX_TILES, gt_tiles and gt_sym_workspace_bytes: sd_rows_check.h, with the entries' check
constexpr int GT_KC = 32;                 // k of one staged chunk
constexpr int GT_LDS = GT_KC + 4;         // LDS row stride, floats: rows stay 16-byte aligned, consecutive rows shift by 4 banks

// columns c .. c + 3 of a row (c % 4 == 0), zeros from column d on; nothing at or past d is read
__device__ __forceinline__ f32x4 gt_load4(const float* __restrict__ row, int c, int d) {
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
__device__ __forceinline__ void gt_take(float& bv, int& bi, float v, int i) {
  if (v > bv || (v == bv && i < bi)) {
    bv = v;
    bi = i;
  }
}

// acc <- the products of tile (ti, tj); `lds` holds 2 * GT_T * GT_LDS floats.  Starts with a barrier before it touches LDS; the caller
// puts one after it before LDS is reused.
__device__ __forceinline__ void gt_tile(const float* __restrict__ rows, const long ld, const int n, const int d, const int ti, const int tj,
                                        float* __restrict__ lds, f32x4 (&acc)[4][4], const int tid, const int wm, const int wn,
                                        const int fr, const int fq) {
  // staging role: thread (r0 = tid / 8, g = tid % 8) moves columns 4 g .. 4 g + 3 of rows r0 + 32 i of both operands
  const int g = tid & 7, r0 = tid >> 3;
  const float* pa[4];
  const float* pb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    int m = ti * GT_T + r0 + 32 * i;
    int c = tj * GT_T + r0 + 32 * i;
    m = m < n ? m : n - 1;                  // rows past n read row n - 1; their scores are never taken
    c = c < n ? c : n - 1;
    pa[i] = rows + (size_t)m * ld;
    pb[i] = rows + (size_t)c * ld;
  }
  f32x4 ra[4], rb[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = gt_load4(pa[i], k0 + 4 * g, d);
      rb[i] = gt_load4(pb[i], k0 + 4 * g, d);
    }
  };

#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float* const a_base = lds + (wm * 64 + fr) * GT_LDS;
  const float* const b_base = lds + (GT_T + wn * 64 + fr) * GT_LDS;
  const int nk = (d + GT_KC - 1) / GT_KC;
  fetch(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                        // every wave is done with the previous chunk
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<f32x4*>(&lds[(r0 + 32 * i) * GT_LDS + 4 * g]) = ra[i];
      *reinterpret_cast<f32x4*>(&lds[(GT_T + r0 + 32 * i) * GT_LDS + 4 * g]) = rb[i];
    }
    __syncthreads();
    if (kt + 1 < nk) fetch((kt + 1) * GT_KC);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int off = 16 * h + 4 * fq;
      f32x4 av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const f32x4*>(a_base + i * 16 * GT_LDS + off);
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = *reinterpret_cast<const f32x4*>(b_base + j * 16 * GT_LDS + off);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][r], bv[j][r], acc[i][j], 0, 0, 0);
    }
  }
}

// The symmetric argmax of tile (ti, tj), ti <= tj, whose weights are in acc; cand(i, r, j) says whether the pair of acc[i][j][r] may be
// taken at all (it must be symmetric in the pair).  The row maxima go to slot `slot_row` of row block ti, the column maxima to slot
// `slot_col` of row block tj.  red_v / red_i carry the reduction over the two waves of a row or column.
template <class Cand>
__device__ __forceinline__ void gt_sym_argmax(const f32x4 (&acc)[4][4], const Cand cand, const int ti, const int tj, const int slot_row,
                                              const int slot_col, const int n, const int npad, float (&red_v)[2][GT_T],
                                              int (&red_i)[2][GT_T], float* __restrict__ ws_val, int* __restrict__ ws_idx, const int tid,
                                              const int wm, const int wn, const int fr, const int fq) {
  const int rbase = ti * GT_T + wm * 64, cbase = tj * GT_T + wn * 64;
  const bool diag = ti == tj;
  int col[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) col[j] = cbase + 16 * j + fr;

  // row maxima over the tile's columns -> slot slot_row of row block ti
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = rbase + 16 * i + 4 * fq + r;
      float bv = -INFINITY;
      int bi = INT_MAX;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (col[j] < n && cand(i, r, j) && (!diag || col[j] > row)) gt_take(bv, bi, acc[i][j][r], col[j]);
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        gt_take(bv, bi, ov, oi);
      }
      if (fr == 0) {
        red_v[wn][wm * 64 + 16 * i + 4 * fq + r] = bv;
        red_i[wn][wm * 64 + 16 * i + 4 * fq + r] = bi;
      }
    }
  __syncthreads();
  if (tid < GT_T) {
    float bv = red_v[0][tid];
    int bi = red_i[0][tid];
    gt_take(bv, bi, red_v[1][tid], red_i[1][tid]);
    const size_t at = (size_t)slot_row * npad + (size_t)ti * GT_T + tid;
    ws_val[at] = bv;
    ws_idx[at] = bi == INT_MAX ? -1 : bi;
  }
  __syncthreads();

  // column maxima over the tile's rows = row maxima of the mirrored tile -> slot slot_col of row block tj
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float bv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = rbase + 16 * i + 4 * fq + r;
        if (row < n && cand(i, r, j) && (!diag || row < col[j])) gt_take(bv, bi, acc[i][j][r], row);
      }
#pragma unroll
    for (int o = 16; o < 64; o <<= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      gt_take(bv, bi, ov, oi);
    }
    if (fq == 0) {
      red_v[wm][wn * 64 + 16 * j + fr] = bv;
      red_i[wm][wn * 64 + 16 * j + fr] = bi;
    }
  }
  __syncthreads();
  if (tid < GT_T) {
    float bv = red_v[0][tid];
    int bi = red_i[0][tid];
    gt_take(bv, bi, red_v[1][tid], red_i[1][tid]);
    const size_t at = (size_t)slot_col * npad + (size_t)tj * GT_T + tid;
    ws_val[at] = bv;
    ws_idx[at] = bi == INT_MAX ? -1 : bi;
  }
}

// the slots of row i in ascending column order, strict >: the lowest index among equal maxima
__device__ __forceinline__ void gt_finish(const float* __restrict__ ws_val, const int* __restrict__ ws_idx, const int slots, const int npad,
                                          const int n, int* __restrict__ nn, float* __restrict__ best, const int i) {
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

// the workspace of the symmetric argmax as the kernels see it: `slots` slots of npad values, then as many indices
struct GtSymWs { int npad, slots; float* val; int* idx; };
inline GtSymWs gt_sym_ws(void* ws, int nt, int slots) {
  const int npad = nt * GT_T;
  float* const val = static_cast<float*>(ws);
  return GtSymWs{npad, slots, val, reinterpret_cast<int*>(val + (size_t)slots * npad)};
}
