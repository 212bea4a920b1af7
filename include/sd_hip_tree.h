/*
 * sd_hip_tree.h — from a spanning tree's edges to HDBSCAN's labels, for many recordings in one launch (same shared object as sd_hip.h,
 * a binding table of its own: `_native.TREE_ENTRIES`, version `sd_tree_abi_version()`).
 *
 * speech-diarization_amd/hdbscan_gpu.py builds the minimum spanning tree of the mutual-reachability graph on the device
 * (sd_hip_hdbscan.h).  What follows is O(n log n) work on n - 1 edges, independent per recording: sort the edges, build the
 * single-linkage dendrogram, condense it at min_cluster_size, sum the stabilities, select by excess of mass, label the rows.  This
 * entry does all of it, one workgroup per recording.
 *
 * Conventions as in sd_hip_hdbscan.h: device pointers, asynchronous on `stream`, no allocation and no synchronisation; 0 = ok,
 * negative = error (SD_ERR_* of sd_hip.h, message via sd_last_error()).  Every refusal happens before anything is launched.
 *
 * THE RESULT.  Per recording, with its edges in the order `order = argsort(dist, kind="stable")` (equal distances keep their place in
 * the list), the labels are those of scikit-learn 1.7.2's
 *     tree_to_labels(make_single_linkage(mst[order]), min_cluster_size, "eom", allow_single_cluster, 0.0, None)[0]
 * exactly: the same cluster numbering (ids in breadth-first order of the dendrogram from the root, left before right, at true splits;
 * a label is the rank of its cluster among the selected ids), the same f64 stabilities (lambda = 1.0 / dist by IEEE division, +inf
 * for dist == 0; one addition per condensed-tree entry in condensed-tree order, no fused multiply-add), the same strict comparison
 * in the selection, and the same rule for a single selected root.  Duplicate rows (dist = 0, lambda = +inf, NaN stabilities) go
 * through the same operations and IEEE arithmetic decides.  cluster_selection_epsilon, max_cluster_size, "leaf" and the
 * probabilities are not computed.
 */
#ifndef SD_HIP_TREE_H
#define SD_HIP_TREE_H

#include "sd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The version moves when an existing entry changes its signature or its meaning. */
#define SD_TREE_ABI_VERSION 1

int sd_tree_abi_version(void);

/*   lo, hi       device int32 [n_edges]: the two rows of every edge, counted from the recording's first row
 *   dist         device f64 [n_edges], 8-byte aligned: finite and >= 0 (0 is legal; -0.0 counts as 0)
 *   first_edge   device int32 [n_groups + 1]: non-decreasing, first_edge[0] = 0, first_edge[n_groups] = n_edges.  Recording g owns the
 *                edges [first_edge[g], first_edge[g + 1]), at least one, and has one more row than edges
 *   max_edges    the caller's upper bound on the edges of any one recording, >= 1
 *   min_cluster_size >= 2;  allow_single_cluster 0 or 1
 *   labels       device int32 [n_edges + n_groups]: the rows of recording g start at first_edge[g] + g; -1 is noise
 *   bad          device int32 [n_groups], written for every recording: 0 = ok; non-zero when the recording's edges are not a spanning
 *                tree of its rows (an index outside [0, n_g), an edge inside one component, no edge at all, more than max_edges
 *                edges), when one of its distances is negative or not finite, or when `first_edge` breaks its promise ANYWHERE (the
 *                workspace slices and the label ranges of the recordings are only disjoint under that promise, so every recording of
 *                the launch is bad then, and all of `labels` is -1).  The labels of a bad recording are all -1; every other recording
 *                is unaffected
 *   ws           device, at least sd_tree_labels_workspace_bytes(n_edges, n_groups, max_edges) bytes, 16-byte aligned; may be null
 *                when that is 0
 *
 * No load or store address depends on unchecked contents of lo, hi or first_edge: every index is compared with its range before it
 * is used, and a value out of range is reported through `bad`.  Every loop carries a bound derived from the recording's size (the
 * union-find walks and the queue walks included); running out of a bound sets `bad` and ends the work.  No atomics: results are
 * bitwise equal run to run.
 *
 * One launch, grid.x = n_groups, 256 threads.  The sort (a bitonic network over (bits of dist, position), all keys distinct) and the
 * labelling of the rows use every thread; the dendrogram, the condensed tree, the stabilities and the selection are sequential and run
 * on one lane while the others wait at a barrier.
 *
 * The state of a recording of n rows is 72 n bytes (8 n sort keys, 8 n stabilities, 14 n int32: the sorted order, the dendrogram's
 * left / right / size, 2 n of union-find parents that later hold the queue of a pruned subtree, the queue of the live nodes, the cluster
 * of a node, the node a row fell out at, and four per-cluster arrays).  It lives in LDS while the recording fits,
 *     SD_TREE_LDS_ROWS = (160 KB - 256) / 72 = 2272 rows,
 * and in the recording's slice of `ws` (72 (first_edge[g] + g) bytes in) above that; the code is the same over either pointer.
 *
 *     sd_tree_labels_workspace_bytes(n_edges, n_groups, max_edges) = 0                            for max_edges + 1 <= 2272
 *                                                                    72 (n_edges + n_groups)      otherwise;
 *                                                                    0 for n_groups <= 0, n_edges < n_groups or max_edges <= 0
 *
 * SD_ERR_ARG: n_groups <= 0, n_edges < n_groups, max_edges <= 0, min_cluster_size < 2, allow_single_cluster not 0 or 1, a null
 * pointer (ws only when bytes are needed), dist not 8-byte aligned, ws not 16-byte aligned.  SD_ERR_UNSUPPORTED: n_edges + n_groups
 * above 2^31 - 1, min(max_edges, n_edges) of 2^30 or more.  SD_ERR_WORKSPACE: a smaller workspace. */
size_t sd_tree_labels_workspace_bytes(int n_edges, int n_groups, int max_edges);
int sd_tree_labels_grouped(const int* lo, const int* hi, const double* dist, const int* first_edge, int n_groups, int n_edges, int max_edges,
                           int min_cluster_size, int allow_single_cluster, int* labels, int* bad, void* ws, size_t ws_bytes,
                           sd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_TREE_H */
