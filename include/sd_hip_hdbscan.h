/*
 * sd_hip_hdbscan.h — the density-clustering entries of libsd_hip.so (same shared object as sd_hip.h, a binding table of their own:
 * `_native.HDBSCAN_PROTOTYPES`, version `sd_hdbscan_abi_version()`).
 *
 * HDBSCAN's only O(N^2) work is the core distance of every row (its min_samples-th nearest neighbour) and a minimum spanning tree of
 * the mutual-reachability graph.  On unit rows both are statements about cosines, and neither needs the N x N matrix:
 *
 *     score(i, j) = <rows[i], rows[j]>                                  (cosine; distance falls as it grows)
 *     core[i]     = the k-th largest score(i, j) over j != i            (k = min_samples - 1: scikit-learn counts the point itself)
 *     w(i, j)     = fminf(fminf(core[i], core[j]), score(i, j))         (mutual reachability, in cosine space)
 *
 * and a Boruvka round of speech-diarization_amd/hdbscan_gpu.py is one call of sd_hdb_outgoing_f32: the heaviest edge that leaves the
 * component of every row.
 *
 * Conventions as in sd_hip_ahc.h: device pointers, asynchronous on `stream`, no allocation and no synchronisation; 0 = ok,
 * negative = error (SD_ERR_* of sd_hip.h, message via sd_last_error()).  Every refusal happens before anything is launched.
 *
 * Precondition of every entry: FINITE rows (the callers check; a NaN score is never selected).  `core` may hold +inf.
 *
 * `rows` is f32 [n][ld] with ld >= d; columns [d, ld) are never read.  Its base must be 16-byte aligned and ld a multiple of 4
 * (SD_ERR_ARG otherwise): full groups of four columns are read with 16-byte loads.
 *
 * THE SCORE.  score(i, j) is an f32 product with f32 accumulation on v_mfma_f32_16x16x4_f32 over 128 x 128 tiles.  Every element of
 * every tile of BOTH entries is produced by the same K loop with the same k order, and a product commutes, so
 *   - score(i, j) and score(j, i) are the same bits, whichever tile and whichever side of the diagonal computes them;
 *   - sd_hdb_core_f32 and sd_hdb_outgoing_f32 see the same bits for the same pair: with all-singleton components and core = +inf,
 *     best[i] of the second IS core[i] of the first at k = 1;
 *   - w(i, j) == w(j, i) bitwise (fminf(core[i], core[j]) commutes, and the mirrored half below reads the same accumulator).
 * The driver's correctness under ties rests on this: with an exactly symmetric w, the edges a Boruvka round chooses under a total
 * order never close a cycle.
 */
#ifndef SD_HIP_HDBSCAN_H
#define SD_HIP_HDBSCAN_H

#include "sd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The version moves when an existing entry changes its signature or its meaning.  An additive entry (the two grouped entries below)
 * does not move it: a caller that needs one looks the symbol up. */
#define SD_HDBSCAN_ABI_VERSION 1

int sd_hdbscan_abi_version(void);

/* core[i] = the k-th largest of the multiset { score(i, j) : j != i } (three equal scores count three times).
 *
 *   rows   device f32 [n][ld], 1 <= d <= 1024 (SD_ERR_UNSUPPORTED above)
 *   k      1 <= k <= 16 (SD_ERR_UNSUPPORTED above 16) and k <= n - 1 (SD_ERR_ARG otherwise; so n >= 2)
 *   core   device f32 [n]
 *   ws     device, at least sd_hdb_core_workspace_bytes(n, d, k) bytes, 16-byte aligned (SD_ERR_WORKSPACE when smaller)
 *
 * One pass over the FULL Gram (both triangles): workgroup (c, I) (grid x = chunk c, grid y = row block I) owns the 128 rows of row
 * block I and walks the column tiles 8 c .. 8 c + 7; two threads per row keep a sorted running top-k in registers, the scores of a tile reach them through LDS.  The k
 * values of chunk c go to slot c of the row; a second kernel merges the C = ceil(T / 8) slots (T = ceil(n / 128)).  The top k of a
 * multiset do not depend on the order its elements are met in: results are bitwise equal run to run.
 *
 *     sd_hdb_core_workspace_bytes(n, d, k) = ceil(T / 8) · 128 T · k · 4       (k scores per slot and padded row);
 *                                            0 for n <= 1, d <= 0, d > 1024, k <= 0, k > 16 or k > n - 1
 *
 * SD_ERR_ARG: a null pointer, n <= 0, d <= 0, k <= 0, k > n - 1, ld < d, rows not 16-byte aligned, ld % 4 != 0, ws not 16-byte aligned.
 * SD_ERR_UNSUPPORTED: d > 1024, k > 16, n > 128 · 65535. */
size_t sd_hdb_core_workspace_bytes(int n, int d, int k);
int sd_hdb_core_f32(const float* rows, long ld, int n, int d, int k, float* core, void* ws, size_t ws_bytes, sd_stream_t stream);

/* For every row i:   best[i] = max of w(i, j) over j with comp[j] != comp[i],    nn[i] = the lowest such j that attains it.
 * A row with no such j (one component) gets nn[i] = -1, best[i] = -inf.
 *
 *   core   device f32 [n]: finite or +inf
 *   comp   device int32 [n]: the component id of each row (any values; only equality is looked at)
 *   nn     device int32 [n]
 *   best   device f32 [n]
 *   ws     device, at least sd_hdb_outgoing_workspace_bytes(n, d) bytes, 16-byte aligned (SD_ERR_WORKSPACE when smaller)
 *
 * The tile, walk, slot layout and finish kernel of sd_ahc_nearest_f32 (sd_hip_ahc.h): 128 x 128 tiles ON AND ABOVE the diagonal only;
 * tile (I, J), I <= J, writes the maxima (w, index) of its rows over its columns into slot [J + 1] of row block I and, from the SAME
 * accumulators, the maxima of its columns over its rows into slot [I] of row block J; the diagonal tile takes j > i for the first and
 * j < i for the second.  Every slot [s][row], 0 <= s <= T, is written exactly once and the columns a slot stands for ascend with s;
 * the finish kernel walks them in ascending order with a strict `>`.  No floating-point atomics: results are bitwise equal run to
 * run.  best[i] == best[nn[i]] bitwise whenever nn[nn[i]] == i.
 *
 *     sd_hdb_outgoing_workspace_bytes(n, d) = (T + 1) · 128 T · 8       (that of sd_ahc_nearest_workspace_bytes);
 *                                             0 for n <= 0, d <= 0 or d > 1024
 *
 * SD_ERR_ARG: a null pointer, n <= 0, d <= 0, ld < d, rows not 16-byte aligned, ld % 4 != 0, ws not 16-byte aligned.
 * SD_ERR_UNSUPPORTED: d > 1024, n > 128 · 65535. */
size_t sd_hdb_outgoing_workspace_bytes(int n, int d);
int sd_hdb_outgoing_f32(const float* rows, long ld, int n, int d, const float* core, const int* comp, int* nn, float* best, void* ws,
                        size_t ws_bytes, sd_stream_t stream);

/* ---- many recordings at once -------------------------------------------------------------------------------------------------------
 * The rows of all recordings stand one after another; a row's core value and every tree edge look only inside the row's own
 * recording.  Conventions as for sd_ahc_nearest_grouped_f32 (sd_hip_ahc.h):
 *
 *   group      device int32 [n]: the recording of every row, NON-DECREASING
 *   max_group  the caller's upper bound on the rows of any one group, >= 1
 *   bad        device int32 [1]: set to 0 first; non-zero afterwards when `group` decreases somewhere or a group has more than
 *              max_group rows (group is monotone, so that is group[i] == group[i + max_group] for some i).  The results mean nothing
 *              then.  No index depends on the contents of `group`: a broken promise is reported and can never send a load or a store
 *              out of bounds
 *
 * Every product comes from the tile of the entries above, with the same k order: the scores of a recording are bit for bit the ones
 * it gets alone, so per group `core`, `nn` minus the group's first row and the bits of `best` equal those of sd_hdb_core_f32 and
 * sd_hdb_outgoing_f32 on the group's rows alone.  No allocation, no synchronisation, no floating-point atomics: results are bitwise
 * equal run to run.  Every refusal happens before anything is launched.
 *
 * The walk is a band.  Rows of one group lie at most max_group - 1 apart, so row block I can meet a row of one of its groups only in
 * the column tiles I - W .. I + W, W = min(T - 1, ceil((max_group - 1) / 128)), T = ceil(n / 128).  A tile outside [0, T) and a tile
 * whose column block shares no group with the row block (decided from two loads of `group`) load nothing. */

/* core[i] = the k-th largest of the multiset { score(i, j) : j != i, group[j] == group[i] } padded with -inf: a row with fewer than k
 * such j gets -inf (hdbscan_gpu.py never asks for it).
 *
 *   k      1 <= k <= 16 (SD_ERR_UNSUPPORTED above 16); there is no k <= n - 1 rule here
 *   ws     device, at least sd_hdb_core_grouped_workspace_bytes(n, d, k, max_group) bytes, 16-byte aligned
 *
 * Grid (ceil((2 W + 1) / 8), T): workgroup (c, I) walks 8 column tiles of the band of row block I over the FULL Gram, I - W + 8 c
 * onwards; the scan, the slots and the merge are those of sd_hdb_core_f32, and the second kernel also checks the two promises.
 *
 *     sd_hdb_core_grouped_workspace_bytes(n, d, k, max_group) = ceil((2 W + 1) / 8) · 128 T · k · 4      (linear in n at a fixed max_group);
 *                                                               0 for n <= 0, d <= 0, d > 1024, k <= 0, k > 16 or max_group <= 0
 *
 * SD_ERR_ARG: a null pointer (group and bad included), n <= 0, d <= 0, ld < d, k <= 0, max_group <= 0, rows not 16-byte aligned,
 * ld % 4 != 0, ws not 16-byte aligned.  SD_ERR_UNSUPPORTED: d > 1024, k > 16, n > 128 · 65535.  SD_ERR_WORKSPACE: a smaller workspace. */
size_t sd_hdb_core_grouped_workspace_bytes(int n, int d, int k, int max_group);
int sd_hdb_core_grouped_f32(const float* rows, long ld, int n, int d, int k, const int* group, int max_group, float* core, int* bad, void* ws,
                            size_t ws_bytes, sd_stream_t stream);

/* best[i] = max of w(i, j) over j with group[j] == group[i] and comp[j] != comp[i],    nn[i] = the lowest such j that attains it, as an
 * index into all n rows.  A row with no such j (its component is its whole group) gets nn[i] = -1, best[i] = -inf.
 *
 *   core, comp, nn, best: as for sd_hdb_outgoing_f32 (component ids need not differ between groups: the group is looked at first)
 *   ws     device, at least sd_hdb_outgoing_grouped_workspace_bytes(n, d, max_group) bytes, 16-byte aligned
 *
 * The grid (T, W + 1), the ownership of the empty tiles, the 2 W + 2 slots of a row block and the workspace are those of
 * sd_ahc_nearest_grouped_f32; the weight is that of sd_hdb_outgoing_f32.
 *
 *     sd_hdb_outgoing_grouped_workspace_bytes(n, d, max_group) = (2 W + 2) · 128 T · 8;
 *                                                                0 for n <= 0, d <= 0, d > 1024 or max_group <= 0
 *
 * SD_ERR_ARG: a null pointer (group and bad included), n <= 0, d <= 0, ld < d, max_group <= 0, rows not 16-byte aligned, ld % 4 != 0,
 * ws not 16-byte aligned.  SD_ERR_UNSUPPORTED: d > 1024, W + 1 > 65535.  SD_ERR_WORKSPACE: a smaller workspace. */
size_t sd_hdb_outgoing_grouped_workspace_bytes(int n, int d, int max_group);
int sd_hdb_outgoing_grouped_f32(const float* rows, long ld, int n, int d, const float* core, const int* comp, const int* group, int max_group,
                                int* nn, float* best, int* bad, void* ws, size_t ws_bytes, sd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_HDBSCAN_H */
