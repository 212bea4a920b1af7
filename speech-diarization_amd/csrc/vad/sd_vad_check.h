// What sd_vad_energy_grouped_f32 and sd_vad_segments_grouped (include/sd_hip_vad.h) refuse, the bytes of the workspace and the sizes of
// the kernels' LDS: CHECK, pure and host-only, in the manner of cut/sd_cut_check.h.  An entry describes its call; the check returns the
// status code and writes the message.  Nothing else is read: no pointer is followed, no environment, no device query.  No HIP header,
// so the same functions compile into a plain C++ program (tests/helpers/vad_check_pure.cpp).
#pragma once
#include <stdio.h>

#include "sd_hip.h"

// ---------------------------------------------------------------- the kernels' layout
constexpr int SD_VAD_E_THREADS = 256;                  // energy: four waves, a frame per wave at a time
constexpr int SD_VAD_E_TILE = 64;                      // frames of `probs` per workgroup
constexpr int SD_VAD_E_STAGE = 12288;                  // floats of LDS for a tile's samples (48 KB): 63 x 160 + 480 = 10 560 fit
constexpr int SD_VAD_S_THREADS = 1024;                 // segments: frames, and runs, per step of a recording's workgroup
constexpr int SD_VAD_S_LDS_RUNS = 8192;                // runs kept in LDS (two int32 each: 64 KB)
constexpr int SD_VAD_S_LDS_FRAMES = 2 * SD_VAD_S_LDS_RUNS - 1;   // (n + 1) / 2 <= 8192: SD_VAD_LDS_FRAMES of the header

// the floats a tile of `count` frames stages, 0 when they do not fit and are read in place
inline long sd_vad_stage_floats(int count, int win, int hop) {
  const long want = (long)(count - 1) * hop + win;
  return count >= 1 && want <= SD_VAD_E_STAGE ? want : 0;
}

// the runs a mask of n frames can hold, which is what a recording's slice of seg_start / seg_end / ws must take
inline int sd_vad_run_capacity(int n) { return n < 0 ? 0 : (n + 1) / 2; }

constexpr size_t SD_VAD_WHY = 224;
#define SD_VAD_NEED(code, cond, ...) do { if (!(cond)) { snprintf(why, SD_VAD_WHY, __VA_ARGS__); return code; } } while (0)

struct SdVadEnergyCall {
  int n_groups, n_frames, win, hop;
  long long n_signal;
  float threshold_db, slope;
  bool table_null;       // first_sample, n_samples, first_frame or bad
  bool frames_null;      // signal or probs (looked at only when n_frames > 0)
};

inline bool sd_vad_finite(float v) { return v - v == 0.f; }

// Every refusal of the energy entry, in order: the numbers, the scorer's parameters, the pointers.
inline int sd_vad_energy_check(const SdVadEnergyCall& c, char* why) {
  const char* const entry = "sd_vad_energy_grouped_f32";
  SD_VAD_NEED(SD_ERR_ARG, c.n_groups > 0 && c.n_frames >= 0 && c.n_signal >= 0, "%s: n_groups=%d n_frames=%d n_signal=%lld", entry, c.n_groups,
              c.n_frames, c.n_signal);
  SD_VAD_NEED(SD_ERR_ARG, c.win >= 1 && c.hop >= 1, "%s: win=%d hop=%d", entry, c.win, c.hop);
  SD_VAD_NEED(SD_ERR_ARG, sd_vad_finite(c.threshold_db) && sd_vad_finite(c.slope), "%s: threshold_db or slope is not finite", entry);
  SD_VAD_NEED(SD_ERR_ARG, !c.table_null && !(c.n_frames > 0 && c.frames_null), "%s: null pointer", entry);
  return SD_OK;
}

struct SdVadSegmentsCall {
  int n_groups, n_frames, seg_cap, open_len, close_len, min_run, max_gap;
  float on, off;
  bool table_null;       // first_frame, first_seg, n_segs or bad
  bool probs_null;       // probs (looked at only when n_frames > 0)
  bool segs_null;        // seg_start, seg_end or ws (looked at only when seg_cap > 0)
  bool ws_misaligned;
  size_t ws_bytes;
};

// the bytes a call of supported numbers needs: a run list, two int32 per run, in every recording's slice
inline size_t sd_vad_segments_need(const SdVadSegmentsCall& c) { return (size_t)8 * (size_t)c.seg_cap; }

// Every refusal of the segments entry, in order: the numbers of the workspace (`numbers_only` stops after them), the thresholds, the
// lengths, the pointers, the workspace.
inline int sd_vad_segments_check(const SdVadSegmentsCall& c, char* why, bool numbers_only = false) {
  const char* const entry = "sd_vad_segments_grouped";
  SD_VAD_NEED(SD_ERR_ARG, c.n_groups > 0 && c.seg_cap >= 0, "%s: n_groups=%d seg_cap=%d", entry, c.n_groups, c.seg_cap);
  if (numbers_only) return SD_OK;
  SD_VAD_NEED(SD_ERR_ARG, c.n_frames >= 0, "%s: n_frames=%d", entry, c.n_frames);
  SD_VAD_NEED(SD_ERR_ARG, c.on > c.off, "%s: on=%g must exceed off=%g (the toggling scan of equal or crossed thresholds stays on the host)", entry,
              (double)c.on, (double)c.off);
  SD_VAD_NEED(SD_ERR_ARG, c.open_len >= 1 && c.close_len >= 1, "%s: open_len=%d close_len=%d", entry, c.open_len, c.close_len);
  SD_VAD_NEED(SD_ERR_ARG, c.min_run >= 0 && c.max_gap >= 0, "%s: min_run=%d max_gap=%d", entry, c.min_run, c.max_gap);
  SD_VAD_NEED(SD_ERR_ARG, !c.table_null && !(c.n_frames > 0 && c.probs_null) && !(c.seg_cap > 0 && c.segs_null), "%s: null pointer", entry);
  if (c.seg_cap == 0) return SD_OK;
  SD_VAD_NEED(SD_ERR_ARG, !c.ws_misaligned, "%s: workspace is not 16-byte aligned", entry);
  const size_t need = sd_vad_segments_need(c);
  SD_VAD_NEED(SD_ERR_WORKSPACE, c.ws_bytes >= need, "%s: workspace of %zu bytes, seg_cap=%d needs %zu", entry, c.ws_bytes, c.seg_cap, need);
  return SD_OK;
}
#undef SD_VAD_NEED

// sd_vad_segments_workspace_bytes: the need of a call whose numbers the check accepts, 0 for every other one
inline size_t sd_vad_workspace_bytes(int seg_cap, int n_groups) {
  SdVadSegmentsCall c = {};
  c.seg_cap = seg_cap, c.n_groups = n_groups;
  char why[SD_VAD_WHY];
  return sd_vad_segments_check(c, why, true) == SD_OK ? sd_vad_segments_need(c) : 0;
}
