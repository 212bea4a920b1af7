/*
 * sd_hip_ahc.h — the agglomerative-clustering entries of libsd_hip.so (same shared object as sd_hip.h, a binding table of their
 * own: `_native.AHC_PROTOTYPES`, version `sd_ahc_abi_version()`).
 *
 * Average-linkage clustering on cosine distance [REF diar_diag.py:218-226] needs no N x N matrix: the linkage between clusters A
 * and B of unit rows is
 *
 *     1 - (1 / (|A| |B|)) · sum over a in A, b in B of <x_a, x_b>  =  1 - <s_A, s_B> / (|A| |B|),     s_A = sum of the rows of A,
 *
 * so a cluster is its row sum and its size, and a merge is one vector add.  Average linkage is reducible: every pair of mutually
 * nearest clusters can be merged in the same round and the dendrogram is still the greedy one.  A round of
 * speech-diarization_amd/ahc_gpu.py is one call of each entry below over the active clusters.
 *
 * Conventions as in sd_hip.h: device pointers, asynchronous on `stream`, no allocation and no synchronisation; 0 = ok,
 * negative = error (SD_ERR_* of sd_hip.h, message via sd_last_error()).  Every refusal happens before anything is launched.
 *
 * Precondition of every entry: FINITE inputs (the callers check; a NaN score is never selected as a maximum).
 *
 * `sums` is f32 [n][ld] with ld >= d; columns [d, ld) are never read or written.  Its base must be 16-byte aligned and ld a
 * multiple of 4 (SD_ERR_ARG otherwise): full groups of four columns are read with 16-byte loads.
 */
#ifndef SD_HIP_AHC_H
#define SD_HIP_AHC_H

#include "sd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SD_AHC_ABI_VERSION 1

int sd_ahc_abi_version(void);

/* For every row i:   score(i, j) = <sums[i], sums[j]> · (inv_count[i] · inv_count[j]),
 *                    best[i] = max over j != i of score(i, j),    nn[i] = the lowest j that attains it (numpy argmax's rule).
 * n == 1: nn[0] = -1, best[0] = -inf.
 *
 *   sums       device f32 [n][ld], 1 <= d <= 1024 (SD_ERR_UNSUPPORTED above)
 *   inv_count  device f32 [n]: 1 / size of the cluster
 *   nn         device int32 [n]
 *   best       device f32 [n]
 *   ws         device, at least sd_ahc_nearest_workspace_bytes(n, d) bytes, 16-byte aligned (SD_ERR_WORKSPACE when smaller)
 *
 * The products run on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation) over 128 x 128 tiles ON AND ABOVE the diagonal
 * only.  The k order of the dot product and the scale expression are the same for every element, and score(j, i) below the diagonal
 * IS the accumulator of score(i, j): scores are exactly symmetric, best[i] == best[nn[i]] bitwise for a reciprocal pair, duplicate
 * rows give bitwise-equal scores.
 *
 * Tile (I, J), I <= J, writes the maxima (score, index) of its rows over its columns into slot [J + 1] of row block I and, from the
 * transposed accumulators, the maxima of its columns over its rows into slot [I] of row block J; the diagonal tile takes j > i for
 * the first and j < i for the second.  Every slot [s][row], 0 <= s <= T, T = ceil(n / 128), is written exactly once, and the
 * columns a slot stands for ascend with s.  A second kernel reduces the T + 1 slots of a row in ascending order with a strict `>`.
 * No floating-point atomics: results are bitwise equal run to run.
 *
 *     sd_ahc_nearest_workspace_bytes(n, d) = (T + 1) · 128 T · 8      (a score and an index per slot and padded row);
 *                                            0 for n <= 0, d <= 0 or d > 1024
 *
 * SD_ERR_ARG: a null pointer, n <= 0, d <= 0, ld < d, sums not 16-byte aligned, ld % 4 != 0, ws not 16-byte aligned.
 * SD_ERR_UNSUPPORTED: d > 1024, n > 128 · 65535. */
size_t sd_ahc_nearest_workspace_bytes(int n, int d);
int sd_ahc_nearest_f32(const float* sums, long ld, int n, int d, const float* inv_count, int* nn, float* best, void* ws,
                       size_t ws_bytes, sd_stream_t stream);

/* One round of merges.  Rows i < j form a pair when nn[i] == j, nn[j] == i and best[i] > cos_thr (the lower row's best decides).
 * For each pair:  sums[i][c] += sums[j][c] (one add per element, c < d),  count[i] += count[j] (f32: exact below 2^24),
 *                 inv_count[i] = 1 / count[i] (correctly rounded),  target[j] = i.
 * Every other row r gets target[r] = r; row j of a pair keeps its sums and counts.  *n_merged (device int32; set to 0 first, then
 * an integer atomic add per pair) is the number of pairs.  One workgroup owns a pair: nothing races, results are bitwise equal run
 * to run.
 *
 *   count, inv_count  device f32 [n];  nn device int32 [n], entries outside [0, n) never pair;  best device f32 [n]
 *   target            device int32 [n]
 *
 * SD_ERR_ARG: a null pointer, n <= 0, d <= 0, ld < d, sums not 16-byte aligned, ld % 4 != 0. */
int sd_ahc_merge_f32(float* sums, long ld, int n, int d, float* count, float* inv_count, const int* nn, const float* best,
                     float cos_thr, int* target, int* n_merged, sd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_AHC_H */
