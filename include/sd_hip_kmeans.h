/*
 * sd_hip_kmeans.h — scikit-learn's k-means labels for many recordings in one launch (same shared object as sd_hip.h, a binding
 * table of its own: `_native.KMEANS_ENTRIES`, version `sd_kmeans_abi_version()`).
 *
 * speech-diarization_amd/cluster_gpu.py leaves the N x k spectral embedding on the device; `sklearn.cluster.k_means(..., n_init=R)`
 * over it was the last step of the spectral route on the host.  Everything random in that call is a fixed number of uniform draws
 * per restart, so the host draws them in advance (speech-diarization_amd/kmeans_gpu.py, `kmeans_draws`) and this entry does the rest:
 * one workgroup per (recording, restart), a second small launch for the selection among the restarts.
 *
 * Conventions as in sd_hip_cut.h: device pointers, asynchronous on `stream`, no allocation and no synchronisation; 0 = ok,
 * negative = error (SD_ERR_* of sd_hip.h, message via sd_last_error()).  Every refusal happens before anything is launched.
 *
 * THE RESULT.  Recording g owns the rows [first_row[g], first_row[g + 1]) of the f64 matrix `rows` [n_rows, dim] with leading
 * dimension ld, n_g of them, and has a cluster count k = k[g], 2 <= k <= max_k <= 32, k < n_g.  With R = n_init restarts,
 * t = 2 + floor(ln k) trials, first[g][r] the row of the first centre of restart r and u[g][r][c][j] (c < k - 1, j < t) uniform
 * numbers in [0, 1), all arithmetic in f64:
 *   1. X = the rows minus their column means; tol = tol_rel x the mean over the columns of the population variance of X.
 *   2. Seeding of restart r (greedy k-means++): c_0 = X[first]; closest_i = |X_i - c_0|^2, pot = sum closest.  For c = 1 .. k - 1
 *      and each trial j: v_j = u pot; cand_j = min(n_g - 1, the number of i whose inclusive prefix sum of `closest` is < v_j);
 *      D_j = min(closest, |X - X[cand_j]|^2), pot_j = sum D_j.  The trial of smallest pot_j, the lowest j among equal ones, becomes
 *      centre c; its D_j and pot_j replace closest and pot.
 *   3. Lloyd, at most max_iter iterations: label_i = argmin_c |X_i - C_c|^2, the lowest c among equal ones; the new centre is the
 *      mean of its rows; shift = sum |C' - C|^2.  Stop "strict" when the labels are those of the iteration before; otherwise stop
 *      when shift <= tol.  After a stop that is not strict, and when the iterations run out, the labels are taken once more against
 *      the final centres.  inertia = sum |X_i - C_label_i|^2.
 *   4. Selection, in restart order: restart r replaces the incumbent when its inertia is strictly lower AND its partition is not
 *      the incumbent's (every cluster of one maps into one cluster of the other: scikit-learn's _is_same_clustering).
 *   5. labels = those of the chosen restart, in that restart's numbering; chosen, inertia, iters = that restart's.
 * This is `sklearn.cluster.k_means(rows_g, k, n_init=R, max_iter=max_iter, tol=tol_rel)` of scikit-learn 1.7 with its random numbers
 * supplied.  The squared distances are sums of squared differences (scikit-learn expands them), and every sum here runs in an order of
 * its own, so the labels are scikit-learn's, integer for integer, wherever no comparison above is decided by less than the rounding of
 * an f64 sum (DESIGN.md section 23 names the margins).
 */
#ifndef SD_HIP_KMEANS_H
#define SD_HIP_KMEANS_H

#include "sd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The version moves when an existing entry changes its signature or its meaning. */
#define SD_KMEANS_ABI_VERSION 1

int sd_kmeans_abi_version(void);

/* The values of a recording's `flags` word (a sum of them); non-zero: the recording's labels are all -1, chosen = -1, inertia = 0,
 * iters = 0.  Every other recording of the launch is unaffected, except under SD_KMEANS_BAD_PROMISE. */
#define SD_KMEANS_EMPTY 1        /* some iteration of some restart left a cluster without rows (scikit-learn relocates rows then) */
#define SD_KMEANS_NONFINITE 2    /* a row holds NaN or inf */
#define SD_KMEANS_BAD_K 4        /* k[g] outside [2, max_k], or k[g] >= n_g */
#define SD_KMEANS_BAD_DRAW 8     /* a first[g][r] outside [0, n_g) */
#define SD_KMEANS_BAD_PROMISE 16 /* `first_row` breaks its promise ANYWHERE: the label ranges of the recordings are only disjoint under
                                    it, so every recording of the launch is flagged and all of `labels` is -1 */

#define SD_KMEANS_MAX_K 32
#define SD_KMEANS_MAX_DIM 32
#define SD_KMEANS_MAX_INIT 16
#define SD_KMEANS_U_STRIDE 155   /* (SD_KMEANS_MAX_K - 1) x 5 doubles per (recording, restart): u[g][r][c][j] at ((g R + r) 31 + c) 5 + j */

/*   rows       device f64 [n_rows, dim], leading dimension ld >= dim (in doubles), 8-byte aligned; row n_rows - 1 ends after dim columns
 *   first_row  device int32 [n_groups + 1]: non-decreasing, first_row[0] = 0, first_row[n_groups] = n_rows
 *   k          device int32 [n_groups]
 *   n_init     R, 1 <= R <= 16;  max_iter >= 1;  tol_rel >= 0 and finite
 *   max_k      2 <= max_k <= 32: a bound on every k[g]; it sizes the workgroup's LDS
 *   max_rows   >= 1: the rows of a recording up to this many are kept in LDS when they fit beside the centres and the partial sums
 *              (160 KB in all); a recording with more rows, or one that does not fit, is read from global memory in every pass.  The
 *              arithmetic is one code path: the bits of the result do not depend on where the rows were read from
 *   first      device int32 [n_groups, n_init]
 *   u          device f64 [n_groups, n_init, 31, 5] (SD_KMEANS_U_STRIDE per restart); only c < k - 1, j < t are read.  Any value is
 *              legal: no address depends on it (a candidate is a count of rows, at most n_g - 1)
 *   labels     device int32 [n_rows]: the rows of recording g start at first_row[g]
 *   chosen, iters, flags   device int32 [n_groups];  inertia  device f64 [n_groups]: written for every recording
 *   ws         device, at least sd_kmeans_grouped_workspace_bytes(n_rows, n_groups, n_init) bytes, 16-byte aligned
 *
 * No load or store address depends on unchecked contents of first_row, k or first: every value is compared with its range before it
 * is used, and a value out of range is reported through `flags`.
 *
 * Two launches.  "kmeans_lloyd_kernel": grid.x = n_groups x n_init, 256 threads, one workgroup per (recording, restart); centres,
 * counts and per-cluster partial sums in LDS, the rows too when they fit.  Every phase uses every thread: the column means, the
 * distances and the argmin (a row per thread), the seeding's block prefix sum with its search, the per-cluster sums (a slice of rows
 * and a column per thread, each with partial sums of its own), the reductions.  "kmeans_select_kernel": grid.x = n_groups, the
 * selection among the restarts and the copy of the chosen labels.  No floating-point atomics (integer atomics on LDS only), no
 * fast-math, and every sum is taken in an order that depends on (n_g, dim, k) alone: two runs give the same bits.
 *
 * The state outside LDS, in `ws`: per restart the seeding's `closest` (f64) and the labels (int32) of every row, and per (recording,
 * restart) the inertia, the iteration count and the flags:
 *
 *     sd_kmeans_grouped_workspace_bytes(n_rows, n_groups, n_init) = 12 n_init n_rows + 16 n_init n_groups;
 *                                                                   0 for n_groups <= 0, n_rows < 0 or n_init outside [1, 16]
 *
 * SD_ERR_ARG: n_groups <= 0, n_rows < 0, dim outside [1, 32], ld < dim, n_init outside [1, 16], max_iter < 1, max_k outside [2, 32],
 * max_rows < 1, tol_rel negative or not finite, a null pointer (rows and labels only when n_rows > 0), rows not 8-byte or ws not
 * 16-byte aligned.  SD_ERR_WORKSPACE: a smaller workspace. */
size_t sd_kmeans_grouped_workspace_bytes(int n_rows, int n_groups, int n_init);
int sd_kmeans_grouped_f64(const double* rows, long ld, int n_rows, int dim, const int* first_row, int n_groups, const int* k, int n_init,
                          int max_iter, double tol_rel, int max_k, int max_rows, const int* first, const double* u, int* labels, int* chosen,
                          double* inertia, int* iters, int* flags, void* ws, size_t ws_bytes, sd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_KMEANS_H */
