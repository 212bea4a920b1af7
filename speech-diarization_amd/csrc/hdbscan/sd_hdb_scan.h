// What the core pass of sd_hdbscan.hip (hdb_core_kernel) and its grouped form (hdbscan/sd_hdb_grouped.hip, hdb_core_grouped_kernel) share:
// the sorted running top-KK of a row and the merge of a row's slots here, as device functions; the scan of a tile's accumulators through
// LDS and the merge of the two threads of a row in sd_hdb_scan_body.h and sd_hdb_halves_body.h, as text that each kernel includes.  The
// kernels stay in their files.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "sd_gram_tile.h"

// HD_MAX_K (16) and HD_CHUNK (8 column tiles per workgroup of the core pass): sd_rows_check.h, with the workspace they size
constexpr int HD_SC = 65;                 // row stride of the score half-tile in LDS: a wave's 64 rows fall into distinct banks
static_assert(GT_T * HD_SC <= 2 * GT_T * GT_LDS, "the score half-tile reuses the staging buffer");
static_assert(GT_T * (HD_MAX_K + 1) <= 2 * GT_T * GT_LDS, "so does the merge of the two threads of a row");

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

// core[i] <- the k-th largest of the chunks * k slot values of row i; nothing for i >= n
template <int KK>
__device__ __forceinline__ void hd_finish(const float* __restrict__ ws, const int chunks, const int npad, const int n, const int k,
                                          float* __restrict__ core, const int i) {
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
