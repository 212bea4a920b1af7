/*
 * sd_hip_turns.h — speaker turns for many recordings at once: window labels to (region, first frame, end frame, label) runs (same
 * shared object as sd_hip.h, a binding table of its own: `_native.TURNS_ENTRIES`, version `sd_turns_abi_version()`).
 *
 * `cluster.relabel_by_first_appearance` followed by `diarization_baseline.labels_to_turns` is the host statement: inside each speech
 * region every frame takes the label of the nearest window centre, and runs of equal labels become turns.
 * speech-diarization_amd/turns_gpu.py drives the entry below and turns the integer runs into the host's rounded times.
 *
 * Conventions as in sd_hip_scd.h: device pointers, asynchronous on `stream`, no allocation and no synchronisation; 0 = ok,
 * negative = error (SD_ERR_* of sd_hip.h, message via sd_last_error()).  Every refusal happens before anything is launched; trouble
 * with one recording comes back in `bad`.  No load or store address depends on unchecked contents of a table.
 */
#ifndef SD_HIP_TURNS_H
#define SD_HIP_TURNS_H

#include "sd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The version moves when an existing entry changes its signature or its meaning. */
#define SD_TURNS_ABI_VERSION 1

int sd_turns_abi_version(void);

/* The values of a recording's `bad` word (a sum of them).  A flagged recording has n_runs = 0 and nothing else of it is written. */
#define SD_TURNS_BAD_LABEL 1   /* a label of the recording is at least its window count: that recording alone */
#define SD_TURNS_BAD_PROMISE 2 /* a promise of rule 4 is broken.  `first_window` or `first_region` broken ANYWHERE: the slices of the
                                  recordings are only disjoint under it, so every recording of the launch is flagged (and its labels
                                  are not looked at).  Anything else (its slice of region_first_window, its centres, its frame counts
                                  or its region starts): that recording alone */

/* A recording's two tables live in LDS while it has at most this many windows, and in its slice of `ws` above that. */
#define SD_TURNS_LDS_WINDOWS 4096

/* ---- Recording g owns the windows [first_window[g], first_window[g + 1]), n of them, and the regions [first_region[g],
 * first_region[g + 1]); region r owns the windows [region_first_window[r], region_first_window[r + 1]) (possibly none) and has
 * n_frames[r] frames.
 *   1. Relabel, per recording: the labels >= 0 are renumbered 0, 1, ... in the order in which they first appear among the recording's
 *      windows; a negative label becomes -1 (`cluster.relabel_by_first_appearance`).  new_labels[w] is the new label of window w.
 *      A label >= n sets SD_TURNS_BAD_LABEL.
 *   2. Frame i of region r lies at t_i = region_start[r] + (i + 0.5) * frame_s in f64, the operations in this order, none contracted.
 *      The owner of frame i is the FIRST window j of the region that minimises |t_i - centre[j]|, the difference and the comparison in
 *      f64.
 *   3. A run is a maximal stretch of a region's frames whose owners carry the same new label.  Runs are emitted in the order of the
 *      regions, then of the frames: run k of recording g is (run_region = the region's index inside the recording, run_first = its
 *      first frame, run_end = one past its last frame, run_label = the new label) at the slots first_window[g] + k; n_runs[g] is
 *      their count; the rest of the slice is left as it was.  A region without windows emits nothing.
 *   4. Promises.  first_window and first_region: non-decreasing, 0 first, n_windows and n_regions last.  For every recording:
 *      region_first_window is non-decreasing over its regions, from first_window[g] to first_window[g + 1]; every n_frames is at least
 *      1; in a region with windows, with t_0 and t_last its first and last frame time and E the largest of |t_0 - c|, |t_last - c|
 *      over its first and last centre c: E is finite, and every centre exceeds the one before it by at least E * 2^-40 (so strictly;
 *      `speech_windows` gives centres at least a sample, 6e-5 s, apart in regions of hours: 1e-8 E).  Under these promises "window j
 *      is nearer to frame i than window j - 1" is false up to some frame f_j and true from it on (the margin keeps the roundings of
 *      two differences apart), f_j does not decrease along a region, and the owner of frame i is the last window with f_j <= i: each
 *      window owns the frames [f_j, f_{j + 1}), possibly none, and a recording has at most as many runs as windows, which is the
 *      capacity of its slice.
 *
 *   first_window, first_region   device int32 [n_recordings + 1]
 *   region_first_window          device int32 [n_regions + 1]
 *   centre                       device f64 [n_windows], seconds: (window start + window length / 2.0) / sample rate
 *   region_start                 device f64 [n_regions], seconds;  n_frames  device int32 [n_regions]: max(1, round((end - start) / frame_s))
 *   labels                       device int32 [n_windows]
 *   new_labels, run_region, run_first, run_end, run_label   device int32 [n_windows]
 *   n_runs, bad                  device int32 [n_recordings]; bad: 0 or a sum of the SD_TURNS_BAD_* above
 *   ws   device, at least sd_turns_workspace_bytes(n_windows, n_recordings) = 8 n_windows bytes when n_windows > SD_TURNS_LDS_WINDOWS
 *        and 0 bytes otherwise (no recording can need it: `ws` is then not looked at), 16-byte aligned
 *
 * One launch, grid.x = n_recordings, 256 threads, one workgroup per recording, labelled "turns_kernel/lds" when the launch needs no
 * workspace and "turns_kernel/ws" when it does.  Per recording: the checks; the first window of every label by an integer minimum
 * into a table, the new numbers by a prefix sum over "this window is the first of its label"; f_j of every window by a binary search
 * over the frames of its region; then, 256 windows at a time with carries, "the last window before this one that owns a frame" by a
 * block scan with the operator max, the heads of the runs from it, their ranks by a prefix sum; at the end every run takes the next
 * head's first frame, or n_frames, as its end.  The work is O(windows x log frames), whatever the regions' lengths.  No
 * floating-point atomics, nothing depends on timing: two runs give the same bytes.
 *
 * SD_ERR_ARG: n_recordings <= 0, n_windows < 0, n_regions < 0, frame_s not finite or not positive, a null pointer (region_start and
 * n_frames when n_regions > 0; the seven [n_windows] arrays when n_windows > 0; ws when the launch needs one), ws not 16-byte aligned.
 * SD_ERR_WORKSPACE: a smaller workspace. */
size_t sd_turns_workspace_bytes(int n_windows, int n_recordings);
int sd_turns_grouped(const int* first_window, const int* first_region, int n_recordings, const int* region_first_window, int n_regions,
                     const double* centre, int n_windows, const double* region_start, const int* n_frames, double frame_s,
                     const int* labels, int* new_labels, int* n_runs, int* run_region, int* run_first, int* run_end, int* run_label,
                     int* bad, void* ws, size_t ws_bytes, sd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_TURNS_H */
