// What sd_turns_grouped (include/sd_hip_turns.h) refuses, the bytes and the layout of its workspace and the constants of the kernel:
// CHECK, pure and host-only, in the manner of scd/sd_scd_check.h.  The entry describes its call; the check returns the status code and
// writes the message.  Nothing else is read: no pointer is followed, no environment, no device query.  No HIP header, so the same
// functions compile into a plain C++ program (tests/helpers/turns_check_pure.cpp).
#pragma once
#include <stdio.h>

#include "sd_hip.h"

// ---------------------------------------------------------------- the kernel's layout
constexpr int SD_TURNS_THREADS = 256;                  // four waves: 256 windows per step of a scan
constexpr int SD_TURNS_T_LDS_WINDOWS = 4096;           // windows of a recording whose two int32 tables stay in LDS: 2 x 16 KB

// The workspace of a launch of n_windows windows: table A int32 [n_windows] | table B int32 [n_windows]; recording g uses the elements
// first_window[g] .. of each.  A launch of at most SD_TURNS_T_LDS_WINDOWS windows has no recording that could need it: 0 bytes.
constexpr size_t sd_turns_ws_b_offset(int n_windows) { return (size_t)4 * (size_t)n_windows; }

constexpr size_t SD_TURNS_WHY = 224;
#define SD_TURNS_NEED(code, cond, ...) do { if (!(cond)) { snprintf(why, SD_TURNS_WHY, __VA_ARGS__); return code; } } while (0)

struct SdTurnsCall {
  int n_recordings, n_regions, n_windows;
  double frame_s;
  bool table_null;       // first_window, first_region, region_first_window, n_runs or bad
  bool region_null;      // region_start or n_frames (looked at only when n_regions > 0)
  bool window_null;      // centre, labels, new_labels, run_region, run_first, run_end or run_label (looked at only when n_windows > 0)
  bool ws_null, ws_misaligned;   // looked at only when the call needs a workspace
  size_t ws_bytes;
};

// the bytes a call of supported numbers needs
inline size_t sd_turns_need(const SdTurnsCall& c) { return c.n_windows > SD_TURNS_T_LDS_WINDOWS ? (size_t)8 * (size_t)c.n_windows : 0; }

// Every refusal of the entry, in order: the numbers of the workspace (`numbers_only` stops after them), the regions, the frame length,
// the pointers, the workspace.
inline int sd_turns_check(const SdTurnsCall& c, char* why, bool numbers_only = false) {
  const char* const entry = "sd_turns_grouped";
  SD_TURNS_NEED(SD_ERR_ARG, c.n_recordings > 0 && c.n_windows >= 0, "%s: n_recordings=%d n_windows=%d", entry, c.n_recordings, c.n_windows);
  if (numbers_only) return SD_OK;
  SD_TURNS_NEED(SD_ERR_ARG, c.n_regions >= 0, "%s: n_regions=%d", entry, c.n_regions);
  SD_TURNS_NEED(SD_ERR_ARG, c.frame_s - c.frame_s == 0.0 && c.frame_s > 0.0, "%s: frame_s is not a positive finite number", entry);
  SD_TURNS_NEED(SD_ERR_ARG, !c.table_null && !(c.n_regions > 0 && c.region_null) && !(c.n_windows > 0 && c.window_null), "%s: null pointer", entry);
  const size_t need = sd_turns_need(c);
  if (need == 0) return SD_OK;
  SD_TURNS_NEED(SD_ERR_ARG, !c.ws_null, "%s: null pointer", entry);
  SD_TURNS_NEED(SD_ERR_ARG, !c.ws_misaligned, "%s: workspace is not 16-byte aligned", entry);
  SD_TURNS_NEED(SD_ERR_WORKSPACE, c.ws_bytes >= need, "%s: workspace of %zu bytes, n_windows=%d needs %zu", entry, c.ws_bytes, c.n_windows, need);
  return SD_OK;
}
#undef SD_TURNS_NEED

// sd_turns_workspace_bytes: the need of a call whose numbers the check accepts, 0 for every other one
inline size_t sd_turns_ws_bytes(int n_windows, int n_recordings) {
  SdTurnsCall c = {};
  c.n_windows = n_windows, c.n_recordings = n_recordings;
  char why[SD_TURNS_WHY];
  return sd_turns_check(c, why, true) == SD_OK ? sd_turns_need(c) : 0;
}
