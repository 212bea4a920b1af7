// The scan of one tile of the core pass: the body of the column-tile loop of hdb_core_kernel<KK> (sd_hdbscan.hip) and of
// hdb_core_grouped_kernel<KK> (hdbscan/sd_hdb_grouped.hip) after gt_tile.  Included INSIDE the loop; the kernel provides
//   acc, lds, top, KK     the tile's accumulators, the staging buffer (reused: 128 rows x 64 columns, stride HD_SC), the thread's top-KK
//   tj, n                 the column tile and the number of rows
//   lrow, half            the scanning role: 32 columns of each 64-column half-tile for row lrow of the row block
//   wm, wn, fr, fq        the lane coordinates of sd_gram_tile.h
//   HD_SCAN_CAND(col, at) whether column col < n, the at-th of the tile, counts for the thread's row
// Text and not a __device__ function, as sd_conv_tile_reg16_body.h is: called as a function, every instantiation of hdb_core_kernel comes
// out with other device code (1 800 to 6 500 changed lines, other register counts), and a shared statement leaves the device code as it
// was (tools/isa_diff.py, profiles/isa_diff_hdb_grouped.json).  No include guard: it is included by both kernels.
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
      const int col0 = tj * GT_T + h * 64 + c0;
      const float* const src = lds + lrow * HD_SC + c0;
      for (int c = 0; c < 32; ++c) {
        const int col = col0 + c;
        if (col < n && HD_SCAN_CAND(col, h * 64 + c0 + c)) hd_insert<KK>(top, src[c]);
      }
    }
