// What an entry that takes "f32 rows" (const float* rows, long ld, int n, int d) refuses, and the bytes of its workspace: CHECK, pure
// and host-only.  The ten entries of sd_ahc.hip, ahc/sd_ahc_grouped.hip, sd_hdbscan.hip, hdbscan/sd_hdb_grouped.hip and diag/sd_diag.hip
// describe their call (SdRowsCall); sd_rows_check returns the status code and writes the message, in the one order every entry has
// always used; the seven *_workspace_bytes functions are sd_rows_workspace_bytes of the same kind and range.  Nothing else is read: no
// pointer is followed, no environment, no device query.  No HIP header, so the same functions compile into a plain C++ program
// (tests/test_rows_check_rules.py).  The geometry the sizes follow from stands here; the kernels read it from here.
#pragma once
#include <stdio.h>

#include "sd_hip.h"
#include "sd_hip_diag.h"

// ---------------------------------------------------------------- the kernels' geometry
constexpr int GT_T = 128;                 // sd_gram_tile.h: tile edge
constexpr int GT_MAX_D = 1024;
constexpr int GT_MAX_TILES = 65535;       // grid.y
constexpr int HD_MAX_K = 16;              // sd_hdbscan.hip: neighbours of a core value
constexpr int HD_CHUNK = 8;               // column tiles per workgroup of the core pass
constexpr int DG_ROWS = SD_WHITEN_ROWS;   // diag/sd_diag.hip: rows per block of partial sums
constexpr int DG_MAX_D = 256;
constexpr int DG_MAX_K = 1024;
inline int dg_tiles(int d) { return (d + 15) / 16; }
inline int dg_blocks(int n) { return (int)(((long)n + DG_ROWS - 1) / DG_ROWS); }

// ---------------------------------------------------------------- host arithmetic (in long / size_t: n, k and max_group up to INT_MAX)
inline int gt_tiles(int n) { return (int)(((long)n + GT_T - 1) / GT_T); }
inline int hd_chunks(int nt) { return (nt + HD_CHUNK - 1) / HD_CHUNK; }
// the banded core pass (hdbscan/sd_hdb_grouped.hip): the chunks of the 2 W + 1 column tiles of a row block
inline int hd_band_chunks(int band) { return (2 * band + 1 + HD_CHUNK - 1) / HD_CHUNK; }
// the banded walk (ahc/sd_ahc_grouped.hip): how many tiles to the right of the diagonal a group of max_group rows can reach, at most nt - 1
inline int ag_band(int nt, int max_group) { const long reach = ((long)max_group - 1 + GT_T - 1) / GT_T; return (int)(reach < nt - 1 ? reach : nt - 1); }
// the workspace of the symmetric argmax: `slots` slots of a (value, index) per padded row.  The full walk has nt + 1, the banded 2 W + 2
inline size_t gt_sym_workspace_bytes(int nt, int slots) { return (size_t)slots * (size_t)nt * GT_T * (sizeof(float) + sizeof(int)); }

// ---------------------------------------------------------------- one call
// SD_ROWS_ONLY    no workspace, no rule of its own: sd_ahc_merge_f32, sd_whiten_apply_f64
// SD_ROWS_LABELS  no workspace; k labels, named in the first message: sd_label_centroids_f32
// SD_ROWS_SYM     the symmetric argmax over every tile: sd_ahc_nearest_f32, sd_hdb_outgoing_f32
// SD_ROWS_BAND    ... over a band; k is max_group: sd_ahc_nearest_grouped_f32, sd_hdb_outgoing_grouped_f32
// SD_ROWS_CORE    the k best of every row: sd_hdb_core_f32
// SD_ROWS_WHITEN  block partials of the f64 statistics: sd_whiten_stats_f64
// SD_ROWS_BAND_CORE  the k best of every row over a band; k and max_group: sd_hdb_core_grouped_f32 (sd_hdb_outgoing_grouped_f32 is _BAND)
enum SdRowsKind { SD_ROWS_ONLY, SD_ROWS_LABELS, SD_ROWS_SYM, SD_ROWS_BAND, SD_ROWS_CORE, SD_ROWS_WHITEN, SD_ROWS_BAND_CORE };
struct SdRowsCall {
  const char *entry, *operand;      // the name in front of every message; what the alignment message calls the rows: "sums", "rows", "x"
  int kind, n, d;
  long ld;
  int min_n, max_d, k;              // min_n 2: the statistics, with their parenthesis.  k: of SD_ROWS_LABELS and _CORE; max_group of _BAND
  struct { const char* name; long v; } more[2];       // further leading dimensions (name null: none); they stand in the first message
  bool any_null, rows_misaligned, ws_misaligned;      // what the entry read off its pointers
  size_t ws_bytes;
  int max_group;                    // of SD_ROWS_BAND_CORE, whose k is k
};

// the bytes a call of supported shape needs (0: the entry has no workspace)
inline size_t sd_rows_need(const SdRowsCall& c) {
  const int nt = gt_tiles(c.n);
  if (c.kind == SD_ROWS_SYM || c.kind == SD_ROWS_BAND) return gt_sym_workspace_bytes(nt, c.kind == SD_ROWS_SYM ? nt + 1 : 2 * ag_band(nt, c.k) + 2);
  if (c.kind == SD_ROWS_CORE) return (size_t)hd_chunks(nt) * (size_t)nt * GT_T * (size_t)c.k * sizeof(float);
  if (c.kind == SD_ROWS_BAND_CORE) return (size_t)hd_band_chunks(ag_band(nt, c.max_group)) * (size_t)nt * GT_T * (size_t)c.k * sizeof(float);
  if (c.kind != SD_ROWS_WHITEN) return 0;
  const size_t T = (size_t)dg_tiles(c.d);
  return (size_t)dg_blocks(c.n) * (16 * T + 256 * (T * (T + 1) / 2)) * sizeof(double);
}

constexpr size_t SD_ROWS_WHY = 192;
#define SD_ROWS_NEED(code, cond, ...) do { if (!(cond)) { snprintf(why, SD_ROWS_WHY, __VA_ARGS__); return code; } } while (0)

// Every refusal of the ten entries, in the order the entries have always made them: the supported range (the rules on the numbers
// alone; `numbers_only` stops after them), the pointers, the rows' alignment and, for an entry with a workspace, its alignment, the grid
// limit and its size.  SD_OK, or the status code with the text in why[SD_ROWS_WHY].
inline int sd_rows_check(const SdRowsCall& c, char* why, bool numbers_only = false) {
  const bool labels = c.kind == SD_ROWS_LABELS;
  const bool more_ok = (!c.more[0].name || c.more[0].v >= c.d) && (!c.more[1].name || c.more[1].v >= c.d);
  if (!(c.n >= c.min_n && c.d > 0 && (!labels || c.k > 0) && c.ld >= c.d && more_ok)) {
    char k[24] = "", more[2][40] = {"", ""}, note[48] = "";
    if (labels) snprintf(k, sizeof(k), " k=%d", c.k);
    for (int i = 0; i < 2; ++i)
      if (c.more[i].name) snprintf(more[i], sizeof(more[i]), " %s=%ld", c.more[i].name, c.more[i].v);
    if (c.min_n > 1) snprintf(note, sizeof(note), " (n >= %d: one row has no covariance)", c.min_n);
    SD_ROWS_NEED(SD_ERR_ARG, false, "%s: n=%d d=%d%s ld=%ld%s%s%s", c.entry, c.n, c.d, k, c.ld, more[0], more[1], note);
  }
  SD_ROWS_NEED(SD_ERR_UNSUPPORTED, c.d <= c.max_d, "%s: d=%d, at most %d columns are supported", c.entry, c.d, c.max_d);
  if (c.kind == SD_ROWS_CORE) SD_ROWS_NEED(SD_ERR_UNSUPPORTED, c.k <= HD_MAX_K, "%s: k=%d, at most %d neighbours are supported", c.entry, c.k, HD_MAX_K);
  if (c.kind == SD_ROWS_CORE) SD_ROWS_NEED(SD_ERR_ARG, c.k >= 1 && c.k <= c.n - 1, "%s: k=%d must lie in 1 .. n - 1 (n=%d)", c.entry, c.k, c.n);
  if (c.kind == SD_ROWS_BAND) SD_ROWS_NEED(SD_ERR_ARG, c.k > 0, "%s: max_group=%d", c.entry, c.k);
  if (c.kind == SD_ROWS_BAND_CORE) {    // no k <= n - 1 rule: a row with fewer than k others in its group gets -inf
    SD_ROWS_NEED(SD_ERR_UNSUPPORTED, c.k <= HD_MAX_K, "%s: k=%d, at most %d neighbours are supported", c.entry, c.k, HD_MAX_K);
    SD_ROWS_NEED(SD_ERR_ARG, c.k >= 1, "%s: k=%d must be at least 1", c.entry, c.k);
    SD_ROWS_NEED(SD_ERR_ARG, c.max_group > 0, "%s: max_group=%d", c.entry, c.max_group);
  }
  if (labels) SD_ROWS_NEED(SD_ERR_UNSUPPORTED, c.k <= DG_MAX_K, "%s: k=%d, at most %d labels are supported", c.entry, c.k, DG_MAX_K);
  if (numbers_only) return SD_OK;
  SD_ROWS_NEED(SD_ERR_ARG, !c.any_null, "%s: null pointer", c.entry);
  SD_ROWS_NEED(SD_ERR_ARG, !c.rows_misaligned && c.ld % 4 == 0, "%s: %s must be 16-byte aligned with ld %% 4 == 0 (ld=%ld)", c.entry, c.operand, c.ld);
  if (c.kind < SD_ROWS_SYM) return SD_OK;       // no workspace
  SD_ROWS_NEED(SD_ERR_ARG, !c.ws_misaligned, "%s: workspace is not 16-byte aligned", c.entry);
  const int nt = gt_tiles(c.n);
  if (c.kind == SD_ROWS_SYM || c.kind == SD_ROWS_CORE || c.kind == SD_ROWS_BAND_CORE)
    SD_ROWS_NEED(SD_ERR_UNSUPPORTED, nt <= GT_MAX_TILES, "%s: n=%d, at most %d rows are supported", c.entry, c.n, GT_MAX_TILES * GT_T);
  if (c.kind == SD_ROWS_BAND)
    SD_ROWS_NEED(SD_ERR_UNSUPPORTED, ag_band(nt, c.k) < GT_MAX_TILES, "%s: max_group=%d, a group of at most %d rows is supported", c.entry, c.k, (GT_MAX_TILES - 1) * GT_T);
  const size_t need = sd_rows_need(c);
  char k[32] = "";
  if (c.kind == SD_ROWS_BAND || c.kind == SD_ROWS_CORE) snprintf(k, sizeof(k), c.kind == SD_ROWS_BAND ? " max_group=%d" : " k=%d", c.k);
  if (c.kind == SD_ROWS_BAND_CORE) snprintf(k, sizeof(k), " k=%d max_group=%d", c.k, c.max_group);
  SD_ROWS_NEED(SD_ERR_WORKSPACE, c.ws_bytes >= need, "%s: workspace of %zu bytes, n=%d d=%d%s needs %zu", c.entry, c.ws_bytes, c.n, c.d, k, need);
  return SD_OK;
}
#undef SD_ROWS_NEED

// *_workspace_bytes(n, d[, k | max_group]): the need of a call whose numbers the check accepts, 0 for every other one.  A size function
// has no leading dimension; d stands in.
inline size_t sd_rows_workspace_bytes(int kind, int n, int d, int min_n, int max_d, int k = 0, int max_group = 0) {
  SdRowsCall c = {"", "", kind, n, d, d, min_n, max_d, k};
  c.max_group = max_group;
  char why[SD_ROWS_WHY];
  return sd_rows_check(c, why, true) == SD_OK ? sd_rows_need(c) : 0;
}

// the library's wrapper (sd_api.hip): the call as the entry describes it plus what its pointers say -> SD_OK, or the refusal with
// sd_last_error set.  An entry without a workspace passes none.
int sd_rows_refused(SdRowsCall c, const void* rows, bool any_null, const void* ws = nullptr, size_t ws_bytes = 0);
