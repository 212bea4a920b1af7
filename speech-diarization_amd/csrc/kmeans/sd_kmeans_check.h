// What sd_kmeans_grouped_f64 (include/sd_hip_kmeans.h) refuses, the bytes of its workspace and the layout of the workgroup's LDS:
// CHECK, pure and host-only, in the manner of cut/sd_cut_check.h.  The entry describes its call (SdKmeansCall); sd_kmeans_check returns
// the status code and writes the message.  Nothing else is read: no pointer is followed, no environment, no device query.  No HIP
// header, so the same functions compile into a plain C++ program (tests/helpers/kmeans_check_pure.cpp).
#pragma once
#include <stdio.h>

#include "sd_hip.h"

struct SdKmeansCall {
  int n_rows, dim, n_groups, n_init, max_iter, max_k, max_rows;
  long ld;
  double tol_rel;
  bool table_null;       // first_row, k, first, u, chosen, inertia, iters, flags or ws
  bool rows_null;        // rows or labels (looked at only when n_rows > 0)
  bool rows_misaligned, ws_misaligned;
  size_t ws_bytes;
};

// ---------------------------------------------------------------- the kernel's layout
constexpr int SD_KM_THREADS = 256;
constexpr int SD_KM_MAX_K = 32, SD_KM_MAX_DIM = 32, SD_KM_MAX_INIT = 16, SD_KM_TRIALS = 5;
constexpr int SD_KM_LDS_BYTES = 160 * 1024;            // of a CU
constexpr int SD_KM_LDS_STATIC = 1024;                 // kept for the kernel's static words

// the row slices of the per-cluster sums: thread (s, j) adds column j of the rows s, s + S, ... into partial sums of its own
constexpr int sd_km_slices(int dim) { return SD_KM_THREADS / dim; }

// the doubles of LDS before the rows: the centres, the partial sums, the column means, the candidates of a seeding step
inline int sd_km_fixed_doubles(int dim, int max_k) { return max_k * dim + sd_km_slices(dim) * max_k * dim + dim + SD_KM_TRIALS * dim; }

// the doubles of LDS a recording's rows may take: column j of row i at j (n | 1) + i (an odd stride: no bank conflicts either way)
inline int sd_km_rows_cap(int dim, int max_k, int max_rows) {
  const long room = (SD_KM_LDS_BYTES - SD_KM_LDS_STATIC) / 8 - sd_km_fixed_doubles(dim, max_k);
  const long want = (long)dim * ((long)max_rows | 1);
  return (int)(want <= room ? want : 0);
}

// the bytes a call of supported numbers needs: per restart `closest` (f64) and the labels (int32) of every row, per (recording,
// restart) the inertia (f64), the iterations and the flags (int32)
inline size_t sd_kmeans_need(const SdKmeansCall& c) {
  return (size_t)12 * (size_t)c.n_init * (size_t)c.n_rows + (size_t)16 * (size_t)c.n_init * (size_t)c.n_groups;
}

constexpr size_t SD_KMEANS_WHY = 224;
#define SD_KMEANS_NEED(code, cond, ...) do { if (!(cond)) { snprintf(why, SD_KMEANS_WHY, __VA_ARGS__); return code; } } while (0)

// Every refusal, in order: the numbers of the workspace (`numbers_only` stops after them), the other numbers, the tolerance, the
// pointers, the alignment, the workspace.
inline int sd_kmeans_check(const SdKmeansCall& c, char* why, bool numbers_only = false) {
  const char* const entry = "sd_kmeans_grouped_f64";
  SD_KMEANS_NEED(SD_ERR_ARG, c.n_groups > 0 && c.n_rows >= 0, "%s: n_groups=%d n_rows=%d", entry, c.n_groups, c.n_rows);
  SD_KMEANS_NEED(SD_ERR_ARG, c.n_init >= 1 && c.n_init <= SD_KM_MAX_INIT, "%s: n_init=%d outside [1, %d]", entry, c.n_init, SD_KM_MAX_INIT);
  if (numbers_only) return SD_OK;
  SD_KMEANS_NEED(SD_ERR_ARG, c.dim >= 1 && c.dim <= SD_KM_MAX_DIM, "%s: dim=%d outside [1, %d]", entry, c.dim, SD_KM_MAX_DIM);
  SD_KMEANS_NEED(SD_ERR_ARG, c.ld >= c.dim, "%s: ld=%ld is less than dim=%d", entry, c.ld, c.dim);
  SD_KMEANS_NEED(SD_ERR_ARG, c.max_iter >= 1, "%s: max_iter=%d", entry, c.max_iter);
  SD_KMEANS_NEED(SD_ERR_ARG, c.max_k >= 2 && c.max_k <= SD_KM_MAX_K, "%s: max_k=%d outside [2, %d]", entry, c.max_k, SD_KM_MAX_K);
  SD_KMEANS_NEED(SD_ERR_ARG, c.max_rows >= 1, "%s: max_rows=%d", entry, c.max_rows);
  SD_KMEANS_NEED(SD_ERR_ARG, c.tol_rel >= 0 && c.tol_rel <= 1.7976931348623157e308, "%s: tol_rel is negative or not finite", entry);
  SD_KMEANS_NEED(SD_ERR_ARG, !c.table_null && !(c.n_rows > 0 && c.rows_null), "%s: null pointer", entry);
  SD_KMEANS_NEED(SD_ERR_ARG, !(c.n_rows > 0 && c.rows_misaligned), "%s: rows are not 8-byte aligned", entry);
  SD_KMEANS_NEED(SD_ERR_ARG, !c.ws_misaligned, "%s: workspace is not 16-byte aligned", entry);
  const size_t need = sd_kmeans_need(c);
  SD_KMEANS_NEED(SD_ERR_WORKSPACE, c.ws_bytes >= need, "%s: workspace of %zu bytes, n_rows=%d n_groups=%d n_init=%d needs %zu", entry, c.ws_bytes,
                 c.n_rows, c.n_groups, c.n_init, need);
  return SD_OK;
}
#undef SD_KMEANS_NEED

// sd_kmeans_grouped_workspace_bytes: the need of a call whose numbers the check accepts, 0 for every other one
inline size_t sd_kmeans_workspace_bytes(int n_rows, int n_groups, int n_init) {
  SdKmeansCall c = {};
  c.n_rows = n_rows, c.n_groups = n_groups, c.n_init = n_init;
  char why[SD_KMEANS_WHY];
  return sd_kmeans_check(c, why, true) == SD_OK ? sd_kmeans_need(c) : 0;
}
