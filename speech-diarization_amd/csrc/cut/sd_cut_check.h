// What sd_ahc_cut_grouped (include/sd_hip_cut.h) refuses, and the bytes of its workspace: CHECK, pure and host-only, in the manner of
// tree/sd_tree_check.h.  The entry describes its call (SdCutCall); sd_cut_check returns the status code and writes the message.
// Nothing else is read: no pointer is followed, no environment, no device query.  No HIP header, so the same functions compile into a
// plain C++ program (tests/helpers/cut_check_pure.cpp).
#pragma once
#include <stdio.h>

#include "sd_hip.h"

struct SdCutCall {
  int n_groups, n_merges, n_rows;
  float cos_thr;
  bool table_null;       // first_merge, first_row, min_clusters, max_clusters, clusters or bad
  bool merges_null;      // lo, hi or key (looked at only when n_merges > 0)
  bool rows_null;        // labels (looked at only when n_rows > 0)
  bool ws_null, ws_misaligned;
  size_t ws_bytes;
};

// the bytes a call of supported numbers needs: `parent`, one int32 per row
inline size_t sd_cut_need(const SdCutCall& c) { return (size_t)4 * (size_t)c.n_rows; }

constexpr size_t SD_CUT_WHY = 192;
#define SD_CUT_NEED(code, cond, ...) do { if (!(cond)) { snprintf(why, SD_CUT_WHY, __VA_ARGS__); return code; } } while (0)

// Every refusal, in order: the numbers (`numbers_only` stops after them), the threshold, the pointers, the workspace.
inline int sd_cut_check(const SdCutCall& c, char* why, bool numbers_only = false) {
  const char* const entry = "sd_ahc_cut_grouped";
  SD_CUT_NEED(SD_ERR_ARG, c.n_groups > 0 && c.n_rows >= 0 && c.n_merges >= 0, "%s: n_groups=%d n_merges=%d n_rows=%d", entry, c.n_groups, c.n_merges,
              c.n_rows);
  SD_CUT_NEED(SD_ERR_ARG, c.n_merges <= c.n_rows, "%s: n_merges=%d exceeds n_rows=%d (a recording of n rows has at most n - 1 merges)", entry,
              c.n_merges, c.n_rows);
  if (numbers_only) return SD_OK;
  SD_CUT_NEED(SD_ERR_ARG, c.cos_thr == c.cos_thr, "%s: cos_thr is not a number", entry);
  SD_CUT_NEED(SD_ERR_ARG, !c.table_null && !(c.n_merges > 0 && c.merges_null) && !(c.n_rows > 0 && (c.rows_null || c.ws_null)), "%s: null pointer",
              entry);
  if (c.n_rows == 0) return SD_OK;
  SD_CUT_NEED(SD_ERR_ARG, !c.ws_misaligned, "%s: workspace is not 16-byte aligned", entry);
  const size_t need = sd_cut_need(c);
  SD_CUT_NEED(SD_ERR_WORKSPACE, c.ws_bytes >= need, "%s: workspace of %zu bytes, n_rows=%d needs %zu", entry, c.ws_bytes, c.n_rows, need);
  return SD_OK;
}
#undef SD_CUT_NEED

// sd_ahc_cut_workspace_bytes: the need of a call whose numbers the check accepts (the merges do not count: n_merges = 0), 0 for every
// other one
inline size_t sd_cut_workspace_bytes(int n_rows, int n_groups) {
  SdCutCall c = {};
  c.n_groups = n_groups, c.n_rows = n_rows;
  char why[SD_CUT_WHY];
  return sd_cut_check(c, why, true) == SD_OK ? sd_cut_need(c) : 0;
}
