// The end of the core pass: the two threads of a row merge, and slot [chunk blockIdx.x][q][padded row] gets the k best of this chunk.
// Included INSIDE hdb_core_kernel<KK> and hdb_core_grouped_kernel<KK> after the column-tile loop, text for the reason
// sd_hdb_scan_body.h gives; the kernel provides top, KK, lds, lrow, half, row, k, ws and npad.
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
