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

/* The version moves when an existing entry changes its signature or its meaning.  An additive entry (the grouped nearest below) does
 * not move it: a caller that needs one looks the symbol up. */
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

/* sd_ahc_nearest_f32 for many recordings at once: the rows of all recordings stand one after another and a cluster never looks
 * outside its own recording.
 *
 *     best[i] = max over j != i with group[j] == group[i] of score(i, j),    nn[i] = the lowest such j, as an index into all n rows.
 *     A row alone in its group: nn[i] = -1, best[i] = -inf.
 *
 *   group      device int32 [n]: the recording of every row, NON-DECREASING
 *   max_group  the caller's upper bound on the rows of any one group, >= 1
 *   bad        device int32 [1]: set to 0 first; non-zero afterwards when `group` decreases somewhere or a group has more than
 *              max_group rows (group is monotone, so that is group[i] == group[i + max_group] for some i).  nn and best mean nothing
 *              then: a broken promise is reported, never answered with silently wrong neighbours
 *   sums, inv_count, nn, best, ws: as for sd_ahc_nearest_f32, with the workspace size below
 *
 * The score, the tile, the k order and the tie rule are those of sd_ahc_nearest_f32: the scores of a recording are bit for bit the
 * ones it gets alone (its nn shifted by its first row), exactly symmetric, best[i] == best[nn[i]] bitwise for a reciprocal pair.  No
 * floating-point atomics: results are bitwise equal run to run.
 *
 * The walk is a band.  Rows of one group lie at most max_group - 1 apart, so tile (I, J), I <= J, can hold a candidate only for
 * J - I <= W = min(T - 1, ceil((max_group - 1) / 128)), T = ceil(n / 128).  T · (W + 1) workgroups are launched; one whose row block
 * and column block share no group (group[last row of I] != group[first row of J]) loads nothing and writes empty slots.  A row block
 * has 2 W + 2 slots in ascending column order: W + 1 for the tiles to its left and the lower half of its diagonal tile, W + 1 for
 * the upper half of its diagonal tile and the tiles to its right; every slot is written exactly once, and a second kernel walks them
 * with a strict `>` and checks the two promises about `group`.  Work and workspace are linear in n at a fixed max_group:
 *
 *     sd_ahc_nearest_grouped_workspace_bytes(n, d, max_group) = (2 W + 2) · 128 T · 8;
 *                                                               0 for n <= 0, d <= 0, d > 1024 or max_group <= 0
 *
 * SD_ERR_ARG: a null pointer (group and bad included), n <= 0, d <= 0, ld < d, max_group <= 0, sums not 16-byte aligned, ld % 4 != 0,
 * ws not 16-byte aligned.  SD_ERR_UNSUPPORTED: d > 1024, W + 1 > 65535.  SD_ERR_WORKSPACE: a workspace smaller than the formula. */
size_t sd_ahc_nearest_grouped_workspace_bytes(int n, int d, int max_group);
int sd_ahc_nearest_grouped_f32(const float* sums, long ld, int n, int d, const float* inv_count, const int* group, int max_group, int* nn,
                               float* best, int* bad, void* ws, size_t ws_bytes, sd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_AHC_H */
