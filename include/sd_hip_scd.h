/*
 * sd_hip_scd.h — speaker-change detection for the segments of many recordings at once: window embeddings to split pieces (same shared
 * object as sd_hip.h, a binding table of its own: `_native.SCD_ENTRIES`, version `sd_scd_abi_version()`).
 *
 * Pass 2 of `anti_stick_diarize.scd_split_segments` is the host statement: the cosine of adjacent window embeddings, the z-score of
 * their distances, `scipy.signal.find_peaks(z, height=thr)`, the cut times and the greedy filter that keeps pieces of at least
 * min_speech_s.  speech-diarization_amd/scd_gpu.py drives the entry below.
 *
 * Conventions as in sd_hip_vad.h: device pointers, asynchronous on `stream`, no allocation and no synchronisation; 0 = ok,
 * negative = error (SD_ERR_* of sd_hip.h, message via sd_last_error()).  Every refusal happens before anything is launched; trouble
 * with one segment comes back in `bad`.  No load or store address depends on unchecked contents of a table.
 */
#ifndef SD_HIP_SCD_H
#define SD_HIP_SCD_H

#include "sd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The version moves when an existing entry changes its signature or its meaning. */
#define SD_SCD_ABI_VERSION 1

int sd_scd_abi_version(void);

/* The values of a segment's `bad` word (a sum of them). */
#define SD_SCD_BAD_CAPACITY 1 /* first_piece[g + 1] - first_piece[g] < max(1, n / 2): the segment emits nothing (n_peaks = n_pieces = 0,
                                 its `sims` NaN, its `peak_mask` 0) */
#define SD_SCD_BAD_PROMISE 2  /* `first_row` or `first_piece` breaks its promise ANYWHERE: the slices of the segments are only disjoint
                                 under it, so every segment of the launch is flagged (every count 0, all of `sims` NaN, all of
                                 `peak_mask` 0) */

/* A segment's distances, cuts and chain live in LDS while it has at most this many rows, and in its slice of `ws` above that. */
#define SD_SCD_LDS_ROWS 2048

/* ---- Segment g owns rows[first_row[g] .. first_row[g + 1]), n rows of `dim` floats `ld` apart, and has m = n - 1 distances.
 *   1. n < 3: n_peaks = 0 and ONE piece (seg_start[g], seg_end[g]), whatever min_speech_s is.
 *   2. s_i = the cosine of rows i and i + 1 in f32: the bits sd_adjacent_cosine_f32 gives for the same rows and eps (one device
 *      function, sd_wave_pair_cosine).  `sims`, when not null: sims[first_row[g] + i] = s_i, the segment's last slot NaN.
 *   3. d_i = 1.f - s_i in f32.  mean = their mean and std = their population standard deviation, both in f64, two passes; thread t of
 *      256 adds the elements t, t + 256, ... in that order, the 64 partial sums of a wave meet in a butterfly and the four waves are
 *      added in order: the order is fixed by m alone, so two runs give the same bits.  z_i = (d_i - mean) / std in f64 when
 *      std > 1e-6, otherwise z_i = d_i (a NaN anywhere makes the comparison false, as on the host).
 *   4. Peaks as scipy.signal.find_peaks(z, height=thr), found on the f32 d_i (z is an increasing map of d): a maximal run [l, r] of
 *      equal values with 1 <= l, r <= m - 2, d[l - 1] < d[l], d[r + 1] < d[r]; its index is p = (l + r) / 2 (integer division); it
 *      is kept iff z[p] >= thr.  n_peaks[g] = the kept peaks; `peak_mask`, when not null, is 1 at first_row[g] + p of each and 0 at
 *      every other row of the segment.
 *   5. No kept peak: ONE piece (seg_start[g], seg_end[g]).
 *   6. cut_j = seg_start[g] + (p_j + 0.5) * hop_ms / 1000.0 in f64, the operations in this order, none contracted.  A cut equal to
 *      the one before it is dropped (the host's `set`).  The cuts are visited in the order of their peaks, which is the host's sorted
 *      order for hop_ms >= 0 (the chain search below assumes it: for hop_ms < 0 the pieces are those of SOME increasing chain).
 *   7. last = seg_start[g]; for every cut in order: cut - last >= min_speech_s emits (last, cut) and sets last = cut; after the
 *      last cut, seg_end[g] - last >= min_speech_s emits (last, seg_end[g]).  A segment may emit no piece.  The pieces go to
 *      piece_start / piece_end [first_piece[g] ..], n_pieces[g] is their count, the rest of the slice is left as it was.  The times are
 *      the host's f64 values, bit for bit.
 *
 *   rows         device f32, n_rows rows; 4-byte aligned is enough
 *   first_row    device int32 [n_segs + 1]: non-decreasing, first_row[0] = 0, first_row[n_segs] = n_rows
 *   seg_start, seg_end  device f64 [n_segs], seconds
 *   first_piece  device int32 [n_segs + 1]: non-decreasing, first_piece[0] = 0, first_piece[n_segs] = piece_cap; segment g needs
 *                first_piece[g + 1] - first_piece[g] >= max(1, n / 2): it has at most (m - 1) / 2 peaks, and one piece more
 *   n_peaks, n_pieces, bad  device int32 [n_segs]; bad: 0 or a sum of the SD_SCD_BAD_* above
 *   piece_start, piece_end  device f64 [piece_cap]
 *   sims         device f32 [n_rows] or null; peak_mask  device uint8 [n_rows] or null: every element is written exactly once
 *   ws           device, at least sd_scd_split_workspace_bytes(n_rows, n_segs) = 16 n_rows bytes, 16-byte aligned
 *
 * One launch, "scd_split_kernel": grid.x = n_segs, 256 threads, one workgroup per segment.  A wave takes the pairs w, w + 4, ...;
 * rise and fall flags, the start of each run of equal distances (a block scan with the operator "max") and the ranks of the kept
 * peaks (a prefix sum) take 256 distances at a time.  Rule 7 is monotone in the cut: next(j), the first later cut that j would
 * accept, is a binary search that every thread does for its cuts; only the walk along that chain is serial, and it has at most
 * (seg_end - seg_start) / min_speech_s links.  No floating-point atomics, no atomics on global memory, nothing depends on timing:
 * two runs give the same bytes.
 *
 * SD_ERR_ARG: n_segs <= 0, n_rows < 0, piece_cap < 0, dim < 1, ld < dim, hop_ms, min_speech_s or eps not finite, thr NaN (an
 * infinite thr is fine: 1e9 and +inf both switch the stage off), a null pointer (rows and ws when n_rows > 0; piece_start and
 * piece_end when piece_cap > 0; `sims` and `peak_mask` may be null), ws not 16-byte aligned.  SD_ERR_WORKSPACE: a smaller workspace. */
size_t sd_scd_split_workspace_bytes(int n_rows, int n_segs);
int sd_scd_split_grouped_f32(const float* rows, int ld, int dim, int n_rows, const int* first_row, int n_segs, const double* seg_start,
                             const double* seg_end, double hop_ms, double thr, double min_speech_s, float eps, const int* first_piece,
                             int piece_cap, int* n_peaks, int* n_pieces, double* piece_start, double* piece_end, float* sims,
                             unsigned char* peak_mask, int* bad, void* ws, size_t ws_bytes, sd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_SCD_H */
