/*
 * sd_hip_cut.h — from the merge log of average-linkage AHC to the labels at a bounded cluster count, for many recordings in one
 * launch (same shared object as sd_hip.h, a binding table of its own: `_native.CUT_ENTRIES`, version `sd_cut_abi_version()`).
 *
 * speech-diarization_amd/ahc_gpu.py merges mutually nearest clusters round by round (sd_hip_ahc.h).  With speaker-count bounds
 * (`min_clusters`, `max_clusters`) the partition is no longer "every merge above the threshold": it is the dendrogram with its
 * m highest merges applied, m chosen so that the cluster count lands inside the bounds.  The driver logs every merge (the lowest
 * rows of the two clusters and a key); this entry picks the m merges and labels the rows, one workgroup per recording.
 *
 * Conventions as in sd_hip_ahc.h: device pointers, asynchronous on `stream`, no allocation and no synchronisation; 0 = ok,
 * negative = error (SD_ERR_* of sd_hip.h, message via sd_last_error()).  Every refusal happens before anything is launched.
 *
 * THE RESULT.  Recording g owns the rows [first_row[g], first_row[g + 1]), n_g of them (0 and 1 are legal), and the merges
 * [first_merge[g], first_merge[g + 1]), L_g <= max(n_g - 1, 0) of them, in log order (children before parents).  With
 *     c = the number of its merges with key > cos_thr                       (strict, as in sd_ahc_merge_f32)
 *     m = max(0, min(max(c, n_g - max_clusters[g]), n_g - min_clusters[g]))
 * the APPLIED merges are the m first in the order (key descending, position in the log ascending); a key of -0.0 counts as 0.0, and
 * since positions differ the order is total.  The driver's keys never exceed a child's key (it logs min(score, the children's keys)),
 * so with the position as tie-break a parent never precedes its child and the m first are a dendrogram cut.  Each applied merge sets
 * parent[hi] = lo; lo < hi, so this is a forest whose roots are the lowest rows of the clusters.  The label of a row is the rank of
 * its root among the roots in ascending order: numbering by first appearance.  clusters[g] = n_g - m.
 */
#ifndef SD_HIP_CUT_H
#define SD_HIP_CUT_H

#include "sd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The version moves when an existing entry changes its signature or its meaning. */
#define SD_CUT_ABI_VERSION 1

int sd_cut_abi_version(void);

/*   lo, hi       device int32 [n_merges]: the lowest rows of the kept and of the absorbed cluster, counted from the recording's first
 *                row; lo < hi
 *   key          device f32 [n_merges]: finite
 *   first_merge  device int32 [n_groups + 1]: non-decreasing, first_merge[0] = 0, first_merge[n_groups] = n_merges
 *   first_row    device int32 [n_groups + 1]: non-decreasing, first_row[0] = 0, first_row[n_groups] = n_rows
 *   cos_thr      any float but NaN; -inf counts every merge, +inf none
 *   min_clusters, max_clusters   device int32 [n_groups]: 1 <= min <= max; either may exceed n_g (m is clamped at 0)
 *   labels       device int32 [n_rows]: the rows of recording g start at first_row[g]
 *   clusters     device int32 [n_groups], written for every recording: n_g - m; 0 for a bad recording
 *   bad          device int32 [n_groups], written for every recording: 0 = ok; non-zero, and the recording's labels all -1, when
 *                  - a merge has lo >= hi or an index outside [0, n_g),
 *                  - a key is not finite,
 *                  - m > L_g: the log is too short for the maximum,
 *                  - min > max or min < 1,
 *                  - L_g > max(n_g - 1, 0): more merges than a recording of n_g rows can have,
 *                  - a row stands as `hi` of two applied merges with different `lo` (after the scatter and a barrier every applied
 *                    merge reads parent[hi] again; no atomic is needed),
 *                  - `first_merge` or `first_row` breaks its promise ANYWHERE: the label ranges of the recordings are only disjoint
 *                    under that promise, so every recording of the launch is bad then and all of `labels` is -1.
 *                Every other recording is unaffected
 *   ws           device, at least sd_ahc_cut_workspace_bytes(n_rows, n_groups) bytes, 16-byte aligned; may be null when that is 0
 *
 * No load or store address depends on unchecked contents of lo, hi, first_merge or first_row: every index is compared with its range
 * before it is used, and a value out of range is reported through `bad`.  The walk from a row to its root is bounded by n_g steps.
 *
 * One launch, grid.x = n_groups, 256 threads, label "ahc_cut_grouped_kernel".  Every phase uses every thread: the check and the
 * count, the selection, the scatter, the walk to the roots, the prefix sum over the root flags.  The selection is a radix select
 * over the 64-bit composite (inverted order-preserving bits of the key, position): 8 passes of 8 bits, a 256-bin histogram in LDS
 * (integer atomics on LDS only), the merges streamed from global memory in every pass, so one code path serves every n_g.  No
 * floating-point atomics and no atomics on global memory: results are bitwise equal run to run.
 *
 * The one piece of state outside LDS is `parent`, one int32 per row, in the recording's slice of `ws` (first_row[g] ints in):
 *
 *     sd_ahc_cut_workspace_bytes(n_rows, n_groups) = 4 n_rows;      0 for n_groups <= 0 or n_rows < 0
 *
 * SD_ERR_ARG: n_groups <= 0, n_rows < 0, n_merges < 0, n_merges > n_rows, cos_thr NaN, a null pointer (lo, hi, key only when
 * n_merges > 0; labels and ws only when n_rows > 0), ws not 16-byte aligned.  SD_ERR_WORKSPACE: a smaller workspace. */
size_t sd_ahc_cut_workspace_bytes(int n_rows, int n_groups);
int sd_ahc_cut_grouped(const int* lo, const int* hi, const float* key, const int* first_merge, const int* first_row, int n_groups,
                       int n_merges, int n_rows, float cos_thr, const int* min_clusters, const int* max_clusters, int* labels,
                       int* clusters, int* bad, void* ws, size_t ws_bytes, sd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_CUT_H */
