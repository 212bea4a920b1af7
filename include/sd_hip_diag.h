/*
 * sd_hip_diag.h — the entries of libsd_hip.so behind the "VBx-like" diarizer [REF diar_diag.py:187-194, 373-383] (same shared object
 * as sd_hip.h, a binding table of their own: `_native.DIAG_PROTOTYPES`, version `sd_diag_abi_version()`).
 *
 * The reference whitens its embeddings in float64: `np.cov` promotes, then `svd`, then 1 / sqrt(S + 1e-6).  An f32 covariance is
 * wrong by about 1e-7 · lambda_max in absolute terms, which is above that 1e-6 floor as soon as lambda_max > 10.  So the two O(N d^2)
 * parts, the covariance and the transform, run in f64 on the f64 matrix cores (v_mfma_f64_16x16x4_f64); the d x d decomposition
 * between them stays on the host (speech-diarization_amd/diag_gpu.py).  Cluster centres are a mean per label, in f64 as well.
 *
 * Conventions as in sd_hip.h: device pointers, asynchronous on `stream`, no allocation and no synchronisation; 0 = ok,
 * negative = error (SD_ERR_* of sd_hip.h, message via sd_last_error()).  Every refusal happens before anything is launched.
 *
 * Precondition of every entry: FINITE inputs (the callers check).
 *
 * `x` is f32 [n][ld] with ld >= d; columns [d, ld) are never read.  Its base must be 16-byte aligned and ld a multiple of 4
 * (SD_ERR_ARG otherwise), 1 <= d <= 256 (SD_ERR_UNSUPPORTED above).  f32 -> f64 is exact, and every value, product and sum below is
 * f64.  No floating-point atomics anywhere: every result is bitwise equal run to run, and its summation order depends on the shape
 * alone.
 */
#ifndef SD_HIP_DIAG_H
#define SD_HIP_DIAG_H

#include "sd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SD_DIAG_ABI_VERSION 1

int sd_diag_abi_version(void);

/* Rows per block of the statistics kernels: partial sums are formed per block of SD_WHITEN_ROWS rows and added in block order. */
#define SD_WHITEN_ROWS 512

/*   mean[c]    = (sum over i of x[i][c]) / n                                               c < d
 *   gram[a][b] = sum over i of (x[i][a] - mean[a]) (x[i][b] - mean[b])                      a, b < d
 * Two passes, as np.cov: the mean first, then the centred products.  The host divides by n - 1.
 *
 *   mean  device f64 [d]
 *   gram  device f64 [d][ldg], ldg >= d; columns [d, ldg) are never written
 *   ws    device, at least sd_whiten_stats_workspace_bytes(n, d) bytes, 16-byte aligned (SD_ERR_WORKSPACE when smaller)
 *
 * Order of summation (B = ceil(n / SD_WHITEN_ROWS) row blocks, T = ceil(d / 16) column tiles):
 *   column sums   one thread per column adds the rows of its block in ascending order; one thread per column then adds the B block
 *                 sums in ascending order and divides by n;
 *   products      one wave per row block and 16 x 16 tile (I, J), I <= J, feeds four rows per v_mfma_f64_16x16x4_f64 in ascending
 *                 order (rows past n and columns past d enter as zeros); one thread per element then adds the B partial tiles in
 *                 ascending order.
 * Only elements on and above the diagonal are computed; gram[b][a] IS gram[a][b]: exactly symmetric.
 *
 *     sd_whiten_stats_workspace_bytes(n, d) = B · (16 T + 256 · T (T + 1) / 2) · 8;      0 for n < 2, d <= 0 or d > 256
 *
 * SD_ERR_ARG: a null pointer, n < 2, d <= 0, ld < d, ldg < d, x not 16-byte aligned, ld % 4 != 0, ws not 16-byte aligned.
 * SD_ERR_UNSUPPORTED: d > 256. */
size_t sd_whiten_stats_workspace_bytes(int n, int d);
int sd_whiten_stats_f64(const float* x, long ld, int n, int d, double* mean, double* gram, long ldg, void* ws, size_t ws_bytes,
                        sd_stream_t stream);

/*   v = (x[i] - mean) · W          (f64 on v_mfma_f64_16x16x4_f64, the columns of x in ascending groups of four)
 *   out[i] = f32(v / (||v||_2 + eps_add))                                            one rounding to f32
 *
 *   mean  device f64 [d]
 *   w     device f64 [d][ldw], ldw >= d; symmetry is not assumed; columns [d, ldw) are never read
 *   out   device f32 [n][ldo], ldo >= d; columns [d, ldo) are never written
 *
 * ||v||^2 is the sum of the squares, per column tile in ascending order and then over the 16 columns of a tile pairwise.
 *
 * SD_ERR_ARG: a null pointer, n <= 0, d <= 0, ld < d, ldw < d, ldo < d, x not 16-byte aligned, ld % 4 != 0.
 * SD_ERR_UNSUPPORTED: d > 256. */
int sd_whiten_apply_f64(const float* x, long ld, int n, int d, const double* mean, const double* w, long ldw, double eps_add,
                        float* out, long ldo, sd_stream_t stream);

/* For every label c < k:   count[c] = the number of rows i with labels[i] == c,
 *                          m = (sum of those rows, f64, in ascending row order) / count[c],
 *                          out[c] = f32(m / (||m||_2 + eps_add)).
 * A label outside [0, k) (noise, -1) is skipped.  A label without rows gives a zero row and count 0.
 *
 *   labels  device int32 [n]
 *   out     device f32 [k][ldo], ldo >= d; columns [d, ldo) are never written
 *   count   device int32 [k]
 *
 * SD_ERR_ARG: a null pointer, n <= 0, d <= 0, k <= 0, ld < d, ldo < d, x not 16-byte aligned, ld % 4 != 0.
 * SD_ERR_UNSUPPORTED: d > 256, k > 1024. */
int sd_label_centroids_f32(const float* x, long ld, int n, int d, const int* labels, int k, double eps_add, float* out, long ldo,
                           int* count, sd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_DIAG_H */
