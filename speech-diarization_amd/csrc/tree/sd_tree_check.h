// What sd_tree_labels_grouped (include/sd_hip_tree.h) refuses, and the bytes of its workspace: CHECK, pure and host-only, in the manner
// of sd_rows_check.h but a check of its own (the entry takes edge lists, not f32 rows).  The entry describes its call (SdTreeCall);
// sd_tree_check returns the status code and writes the message.  Nothing else is read: no pointer is followed, no environment, no
// device query.  No HIP header, so the same functions compile into a plain C++ program (tests/helpers/tree_check_pure.cpp).  The
// layout the sizes follow from stands here; the kernel reads it from here.
#pragma once
#include <limits.h>
#include <stdio.h>

#include "sd_hip.h"

// ---------------------------------------------------------------- the kernel's layout
constexpr int SD_TREE_ROW_BYTES = 72;                  // 8 sort key + 8 stability + 14 int32 per row of a recording
constexpr int SD_TREE_LDS_BYTES = 160 * 1024;          // of a CU
constexpr int SD_TREE_LDS_STATIC = 256;                // kept for the kernel's few static words
constexpr int SD_TREE_MAX_ROWS = 1 << 30;               // of one recording: the kernel counts its 2 n - 1 nodes in int
constexpr int SD_TREE_LDS_ROWS = (SD_TREE_LDS_BYTES - SD_TREE_LDS_STATIC) / SD_TREE_ROW_BYTES;      // 2272

struct SdTreeCall {
  int n_edges, n_groups, max_edges, min_cluster_size, allow_single_cluster;
  bool any_null, ws_null, dist_misaligned, ws_misaligned;      // what the entry read off its pointers (any_null: ws not counted)
  size_t ws_bytes;
};

// the rows whose state the launch keeps in LDS: the largest recording the caller announces, at most what a CU holds
inline int sd_tree_lds_rows(int max_edges) { return (long)max_edges + 1 <= SD_TREE_LDS_ROWS ? max_edges + 1 : SD_TREE_LDS_ROWS; }

// the bytes a call of supported numbers needs
inline size_t sd_tree_need(const SdTreeCall& c) {
  if ((long)c.max_edges + 1 <= SD_TREE_LDS_ROWS) return 0;
  return (size_t)SD_TREE_ROW_BYTES * ((size_t)c.n_edges + (size_t)c.n_groups);
}

constexpr size_t SD_TREE_WHY = 192;
#define SD_TREE_NEED(code, cond, ...) do { if (!(cond)) { snprintf(why, SD_TREE_WHY, __VA_ARGS__); return code; } } while (0)

// Every refusal, in order: the numbers (`numbers_only` stops after them), the pointers, the alignments, the workspace's size.
inline int sd_tree_check(const SdTreeCall& c, char* why, bool numbers_only = false) {
  const char* const entry = "sd_tree_labels_grouped";
  SD_TREE_NEED(SD_ERR_ARG, c.n_groups > 0 && c.n_edges >= c.n_groups, "%s: n_edges=%d n_groups=%d (every recording has at least one edge)", entry,
               c.n_edges, c.n_groups);
  SD_TREE_NEED(SD_ERR_ARG, c.max_edges > 0, "%s: max_edges=%d", entry, c.max_edges);
  SD_TREE_NEED(SD_ERR_UNSUPPORTED, (long)c.n_edges + c.n_groups <= INT_MAX, "%s: n_edges=%d n_groups=%d, at most %d rows are supported", entry,
               c.n_edges, c.n_groups, INT_MAX);
  SD_TREE_NEED(SD_ERR_UNSUPPORTED, (c.max_edges < c.n_edges ? c.max_edges : c.n_edges) < SD_TREE_MAX_ROWS, "%s: max_edges=%d, a recording of at most %d rows is supported",
               entry, c.max_edges, SD_TREE_MAX_ROWS);
  if (numbers_only) return SD_OK;
  SD_TREE_NEED(SD_ERR_ARG, c.min_cluster_size >= 2, "%s: min_cluster_size=%d must be at least 2", entry, c.min_cluster_size);
  SD_TREE_NEED(SD_ERR_ARG, c.allow_single_cluster == 0 || c.allow_single_cluster == 1, "%s: allow_single_cluster=%d must be 0 or 1", entry,
               c.allow_single_cluster);
  const size_t need = sd_tree_need(c);
  SD_TREE_NEED(SD_ERR_ARG, !c.any_null && !(need && c.ws_null), "%s: null pointer", entry);
  SD_TREE_NEED(SD_ERR_ARG, !c.dist_misaligned, "%s: dist must be 8-byte aligned", entry);
  if (!need) return SD_OK;
  SD_TREE_NEED(SD_ERR_ARG, !c.ws_misaligned, "%s: workspace is not 16-byte aligned", entry);
  SD_TREE_NEED(SD_ERR_WORKSPACE, c.ws_bytes >= need, "%s: workspace of %zu bytes, n_edges=%d n_groups=%d max_edges=%d needs %zu", entry, c.ws_bytes,
               c.n_edges, c.n_groups, c.max_edges, need);
  return SD_OK;
}
#undef SD_TREE_NEED

// sd_tree_labels_workspace_bytes: the need of a call whose numbers the check accepts, 0 for every other one
inline size_t sd_tree_workspace_bytes(int n_edges, int n_groups, int max_edges) {
  const SdTreeCall c = {n_edges, n_groups, max_edges, 2, 0};
  char why[SD_TREE_WHY];
  return sd_tree_check(c, why, true) == SD_OK ? sd_tree_need(c) : 0;
}
