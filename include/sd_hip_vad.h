/*
 * sd_hip_vad.h — voice activity for many recordings at once: frame scores of the stand-in scorer, and frame probabilities to speech
 * runs (same shared object as sd_hip.h, a binding table of its own: `_native.VAD_ENTRIES`, version `sd_vad_abi_version()`).
 *
 * speech-diarization_amd/vad.py is the host statement: `EnergyScorer` over `frame_audio`, then `hysteresis_binarize`,
 * `morph_open_close` and the run logic of `mask_to_segments`.  speech-diarization_amd/vad_gpu.py drives the two entries below and keeps
 * the padding, the clamp and the rounding of `mask_to_segments` on the host (a few hundred integers per hour of audio).
 *
 * Conventions as in sd_hip_cut.h: device pointers, asynchronous on `stream`, no allocation and no synchronisation; 0 = ok,
 * negative = error (SD_ERR_* of sd_hip.h, message via sd_last_error()).  Every refusal happens before anything is launched; trouble
 * with one recording comes back in `bad`.  No load or store address depends on unchecked contents of a table.
 */
#ifndef SD_HIP_VAD_H
#define SD_HIP_VAD_H

#include "sd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The version moves when an existing entry changes its signature or its meaning. */
#define SD_VAD_ABI_VERSION 1

int sd_vad_abi_version(void);

/* The values of a recording's `bad` word (a sum of them). */
#define SD_VAD_SHORT 1        /* energy: n_samples[g] < win */
#define SD_VAD_BAD_RANGE 2    /* energy: the recording's samples do not lie inside [0, n_signal) */
#define SD_VAD_BAD_FRAMES 4   /* energy: first_frame[g + 1] - first_frame[g] is not 1 + (n_samples[g] - win) / hop, or the range leaves
                                 [0, n_frames], or first_frame[0] != 0, or first_frame[n_groups] != n_frames */
#define SD_VAD_BAD_CAPACITY 8 /* segments: first_seg[g + 1] - first_seg[g] < (n_g + 1) / 2 */
#define SD_VAD_BAD_PROMISE 16 /* segments: `first_frame` or `first_seg` breaks its promise ANYWHERE: the slices of the recordings are only
                                 disjoint under it, so every recording of the launch is flagged */

/* ---- Entry 1.  p = sigmoid(slope (20 log10 sqrt(max(mean of squares, 1e-12)) - threshold_db)) of every frame of every recording:
 * `vad.EnergyScorer` over `vad.frame_audio`.
 *
 *   signal        device f32 [n_signal]; 4-byte aligned is enough, and so is any first_sample
 *   first_sample  device int64 [n_groups]; n_samples  device int32 [n_groups]: recording g owns signal[first_sample[g] .. + n_samples[g])
 *   win, hop      >= 1, in samples: frame t of a recording is its samples [t hop, t hop + win); 1 + (n_samples[g] - win) / hop frames
 *   first_frame   device int32 [n_groups + 1]: first_frame[0] = 0, first_frame[g + 1] - first_frame[g] = the frames of recording g,
 *                 first_frame[n_groups] = n_frames
 *   probs         device f32 [n_frames]: EVERY element is written exactly once; the frames of a bad recording, and frames that belong
 *                 to no recording under a broken table, are NaN
 *   bad           device int32 [n_groups]: 0 or a sum of SD_VAD_SHORT, SD_VAD_BAD_RANGE, SD_VAD_BAD_FRAMES
 *
 * One launch, "vad_energy_kernel": grid.x = ceil(n_frames / 64), 256 threads; workgroup b owns the frames [64 b, 64 b + 64) of `probs`.
 * It finds the recording of a frame by a bounded search in first_frame, compares what it read with the ranges above, and stages the
 * samples of its frames of one recording ONCE in LDS ((count - 1) hop + win floats; read from global memory in place when that is
 * more than 12 288).  A wave sums one frame: lane l adds the squares of the samples l, l + 64, ... in f64 (a square of an f32 is exact
 * there), then the 64 partial sums are added in a butterfly: the order depends on (win, hop) alone, never on where the samples were
 * read from, so two runs give the same bits.  The scalar tail is f64, rounded once to f32.  A NaN sample makes NaN for the frames
 * that hold it and for no other.  No atomics.
 *
 * SD_ERR_ARG: n_groups <= 0, n_frames < 0, n_signal < 0, win < 1, hop < 1, slope or threshold_db not finite, a null pointer (signal
 * and probs only when n_frames > 0). */
int sd_vad_energy_grouped_f32(const float* signal, long long n_signal, const long long* first_sample, const int* n_samples, int n_groups,
                              int win, int hop, float threshold_db, float slope, const int* first_frame, int n_frames, float* probs, int* bad,
                              sd_stream_t stream);

/* ---- Entry 2.  Recording g owns probs[first_frame[g] .. first_frame[g + 1]), n_g frames.  In order:
 *   1. hysteresis (`on` > `off`, f32): frame i is speech iff the most recent event at or before i is a start; p >= on is a start,
 *      p < off a stop, so a NaN is no event.  This is `vad.hysteresis_binarize`.
 *   2. opening with a line of open_len: the runs of at least open_len frames stay.
 *   3. closing with a line of L = close_len, c = L / 2: runs less than L frames apart become one; then the frames before c and the
 *      last L - 1 - c frames are cleared (scipy's closing erodes at the borders).  2 and 3 are `vad.morph_open_close`; a length of 1
 *      makes the stage the identity.  `mask`, when not null, receives this mask, one byte (0 or 1) per frame.
 *   4. the runs shorter than min_run frames are dropped, THEN the remaining runs at most max_gap frames apart become one.
 *   5. n_segs[g] = the runs that are left; seg_start / seg_end [first_seg[g] .. + n_segs[g]) their first frame and the frame after
 *      their last, relative to the recording: the `seg_start` / `seg_end` of `vad.mask_to_segments` before padding.  The rest of the
 *      recording's slice is left as it was.
 *
 *   first_frame  device int32 [n_groups + 1]: non-decreasing, first_frame[0] = 0, first_frame[n_groups] = n_frames
 *   first_seg    device int32 [n_groups + 1]: non-decreasing, first_seg[0] = 0, first_seg[n_groups] = seg_cap; recording g needs
 *                first_seg[g + 1] - first_seg[g] >= (n_g + 1) / 2: a mask of n frames has at most that many runs, and no stage makes more
 *   bad          device int32 [n_groups]: 0, SD_VAD_BAD_CAPACITY (n_segs[g] = 0, the recording's mask all 0) or SD_VAD_BAD_PROMISE
 *                (every recording; every n_segs 0, all of `mask` 0)
 *   ws           device, at least sd_vad_segments_workspace_bytes(seg_cap, n_groups) = 8 seg_cap bytes, 16-byte aligned
 *
 * One launch, "vad_segments_kernel": grid.x = n_groups, 1024 threads, one workgroup per recording.  The frames go through a block scan
 * with the operator "last non-zero" 1 024 at a time; run starts and ends are ranked by a prefix sum of their flags and stored as a run
 * list, which every later stage filters, joins or clips in place with one prefix sum per 1 024 runs.  The run list lives in LDS
 * while the recording has at most SD_VAD_LDS_FRAMES frames (8 192 runs of two int32), and in the recording's slice of `ws` above
 * that.  No floating-point atomics, no atomics on global memory, and nothing depends on timing: two runs give the same bytes.
 *
 * SD_ERR_ARG: n_groups <= 0, n_frames < 0, seg_cap < 0, on <= off or either not a number, open_len < 1, close_len < 1, min_run < 0,
 * max_gap < 0, a null pointer (probs when n_frames > 0; seg_start, seg_end and ws when seg_cap > 0; `mask` may be null), ws not
 * 16-byte aligned.  SD_ERR_WORKSPACE: a smaller workspace. */
#define SD_VAD_LDS_FRAMES 16383
size_t sd_vad_segments_workspace_bytes(int seg_cap, int n_groups);
int sd_vad_segments_grouped(const float* probs, const int* first_frame, int n_groups, int n_frames, float on, float off, int open_len,
                            int close_len, int min_run, int max_gap, const int* first_seg, int seg_cap, int* n_segs, int* seg_start,
                            int* seg_end, unsigned char* mask, int* bad, void* ws, size_t ws_bytes, sd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_VAD_H */
