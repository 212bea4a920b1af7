// What sd_scd_split_grouped_f32 (include/sd_hip_scd.h) refuses, the bytes of its workspace, the layout of the workspace and of the
// kernel's LDS: CHECK, pure and host-only, in the manner of vad/sd_vad_check.h.  The entry describes its call; the check returns the
// status code and writes the message.  Nothing else is read: no pointer is followed, no environment, no device query.  No HIP header,
// so the same functions compile into a plain C++ program (tests/helpers/scd_check_pure.cpp).
#pragma once
#include <stdio.h>

#include "sd_hip.h"

// ---------------------------------------------------------------- the kernel's layout
constexpr int SD_SCD_THREADS = 256;                    // four waves: a pair per wave at a time, 256 distances per step of a scan
constexpr int SD_SCD_S_LDS_ROWS = 2048;                // rows of a segment whose distances (f32), cuts (f64) and chain (int32) stay in
constexpr int SD_SCD_S_LDS_CUTS = SD_SCD_S_LDS_ROWS / 2;   // LDS: 8 + 8 + 4 KB; a segment of n rows has at most (n - 2) / 2 cuts

// The workspace of a launch of n_rows rows: cuts f64 [n_rows] | distances f32 [n_rows] | chain int32 [n_rows]; segment g uses the
// elements first_row[g] .. of each (a segment of n rows needs n - 1 distances and at most (n - 2) / 2 cuts and links)
constexpr size_t sd_scd_ws_dist_offset(int n_rows) { return (size_t)8 * (size_t)n_rows; }
constexpr size_t sd_scd_ws_chain_offset(int n_rows) { return (size_t)12 * (size_t)n_rows; }

// the pieces a segment of n rows can emit, which is what its slice of piece_start / piece_end must take
constexpr int sd_scd_piece_capacity(int n) { return n / 2 > 1 ? n / 2 : 1; }

constexpr size_t SD_SCD_WHY = 224;
#define SD_SCD_NEED(code, cond, ...) do { if (!(cond)) { snprintf(why, SD_SCD_WHY, __VA_ARGS__); return code; } } while (0)

struct SdScdCall {
  int ld, dim, n_rows, n_segs, piece_cap;
  double hop_ms, thr, min_speech_s;
  float eps;
  bool table_null;       // first_row, seg_start, seg_end, first_piece, n_peaks, n_pieces or bad
  bool rows_null;        // rows or ws (looked at only when n_rows > 0)
  bool pieces_null;      // piece_start or piece_end (looked at only when piece_cap > 0)
  bool ws_misaligned;
  size_t ws_bytes;
};

inline bool sd_scd_finite(double v) { return v - v == 0.0; }

// the bytes a call of supported numbers needs
inline size_t sd_scd_need(const SdScdCall& c) { return (size_t)16 * (size_t)c.n_rows; }

// Every refusal of the entry, in order: the numbers of the workspace (`numbers_only` stops after them), the capacity, the row shape,
// the parameters, the pointers, the workspace.
inline int sd_scd_check(const SdScdCall& c, char* why, bool numbers_only = false) {
  const char* const entry = "sd_scd_split_grouped_f32";
  SD_SCD_NEED(SD_ERR_ARG, c.n_segs > 0 && c.n_rows >= 0, "%s: n_segs=%d n_rows=%d", entry, c.n_segs, c.n_rows);
  if (numbers_only) return SD_OK;
  SD_SCD_NEED(SD_ERR_ARG, c.piece_cap >= 0, "%s: piece_cap=%d", entry, c.piece_cap);
  SD_SCD_NEED(SD_ERR_ARG, c.dim >= 1 && c.ld >= c.dim, "%s: dim=%d ld=%d", entry, c.dim, c.ld);
  SD_SCD_NEED(SD_ERR_ARG, sd_scd_finite(c.hop_ms) && sd_scd_finite(c.min_speech_s) && sd_scd_finite((double)c.eps),
              "%s: hop_ms, min_speech_s or eps is not finite", entry);
  SD_SCD_NEED(SD_ERR_ARG, c.thr == c.thr, "%s: thr is not a number", entry);
  SD_SCD_NEED(SD_ERR_ARG, !c.table_null && !(c.n_rows > 0 && c.rows_null) && !(c.piece_cap > 0 && c.pieces_null), "%s: null pointer", entry);
  if (c.n_rows == 0) return SD_OK;
  SD_SCD_NEED(SD_ERR_ARG, !c.ws_misaligned, "%s: workspace is not 16-byte aligned", entry);
  const size_t need = sd_scd_need(c);
  SD_SCD_NEED(SD_ERR_WORKSPACE, c.ws_bytes >= need, "%s: workspace of %zu bytes, n_rows=%d needs %zu", entry, c.ws_bytes, c.n_rows, need);
  return SD_OK;
}
#undef SD_SCD_NEED

// sd_scd_split_workspace_bytes: the need of a call whose numbers the check accepts, 0 for every other one
inline size_t sd_scd_workspace_bytes(int n_rows, int n_segs) {
  SdScdCall c = {};
  c.n_rows = n_rows, c.n_segs = n_segs;
  char why[SD_SCD_WHY];
  return sd_scd_check(c, why, true) == SD_OK ? sd_scd_need(c) : 0;
}
