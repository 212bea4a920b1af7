/*
 * sd_hip_trace.h — the launch log of libsd_hip.so, the plan of its ECAPA forward and the choice of its conv entries (same shared object
 * as sd_hip.h, a binding table of its own: `_native.TRACE_PROTOTYPES`, version `sd_trace_abi_version()`).
 *
 * The library chooses among its kernels, their template instantiations and their tile walks on the host, by cost rules, the CU count,
 * sd_set_tuning keys and alignment.  The log makes the choice observable: every kernel launch that succeeded is counted under its
 * LABEL.  A label is the kernel's name, followed by <...> naming the instantiation and /... naming the walk wherever the host chose
 * between several at run time: "conv_gemm_f32_s64_kernel<32>", "seg_mean_std_kernel<f16,packed,64x4>",
 * "conv_gemm_f16_t256_kernel<f16,direct>/lockstep".  The text before the first '<' or '/' is always the __global__ function's name.
 *
 * Host side only.  Counting happens after the launch call returned, in the calling thread, under a process-wide mutex (entries may be
 * called from several threads): no device work, no synchronisation, no stream operation, and no allocation once a label has been
 * counted before.  A launch recorded into a captured graph is counted when it is captured, not when the graph is replayed.  With the
 * log off a launch costs one relaxed atomic load.
 *
 * Whole-process census: with SD_EXPERIMENT=1 and SD_LAUNCH_LOG=<path> in the environment when the library is loaded, every launch of the
 * process is counted (whatever sd_launch_log_enable is told) and the lines of sd_launch_log_read are written to <path> at exit.
 */
#ifndef SD_HIP_TRACE_H
#define SD_HIP_TRACE_H

#include <stddef.h>

#include "sd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SD_TRACE_ABI_VERSION 3

int sd_trace_abi_version(void);

/* on != 0: clear the counts and start counting; on == 0: stop (the counts stay readable).  Returns the previous state (0 / 1). */
int sd_launch_log_enable(int on);

/* The counts since the last sd_launch_log_enable(1) as lines "label\tcount\n", sorted by label, NUL-terminated.  At most cap bytes are
 * written (a truncated text is still terminated; buf may be NULL with cap 0).  Returns the bytes the whole text needs, its NUL
 * included: a result above cap says the buffer was short. */
size_t sd_launch_log_read(char* buf, size_t cap);

/* The plan of one ECAPA forward (csrc/sd_ecapa.hip) as text, without touching a device: what
 * sd_ecapa_forward_* would launch for these weights (geometry, packings, w_dtype, split16), B segments of T frames (map_kind 0: uniform,
 * 1: relative lengths) or B packed spans of M frames in all (map_kind 2; T ignored), 16-byte aligned features, and the tuning and
 * experiment switches as a forward reads them now.  Buffer and return convention of sd_launch_log_read; 0, with sd_last_error() set,
 * where the weights or the shape are refused.
 * The first line is "carve\t-\t\t<the workspace buffers this geometry and mode have, by name>".  Then one line per launch, in order:
 *     step \t route \t reads \t writes
 * step    [b<block>.]<layer>[.<Res2Net step>] with layer one of: cast stem tdnn1 res2 chain tdnn2 squeeze se1 se2 scale mfa stats asp_g
 *         asp_h asp_conv pool fc, or <layer>.pack: the pack pass in front of that layer
 * route   f32              the exact-f32 conv operator (sd_conv1d_cl_f32); which kernel it picks: sd_conv_choice_read
 *         split128         128x128 split kernel, f32 input split while staged, the layer's own bias / scale (w_scale_inv)
 *         split128_folded  the same kernel with the wide packing's folded 2^s vectors (small launches of the C-wide layers)
 *         split256_pack    256x256 split kernel over xs, which the pack step before it wrote
 *         split256_twin    256x256 split kernel over an SD_DT_SPLIT16 tensor its producer wrote
 *         f16              the f16 conv operator (sd_conv1d_cl_f16)
 *         packed           the packed-span conv (sd_conv1d_cl_packed_f32)
 *         seg_gemm         per-segment GEMM (sd_seg_gemm_f32: one launch, or two where it splits K over the grid)
 *         chain            the fused f16 Res2Net chain        cast   features f32 -> f16        pack   f32 -> SD_DT_SPLIT16
 *         asp_fused        attention conv + softmax + statistics in one kernel;  asp_pool: the pooling kernel after a separate asp_conv step
 *         se_scale         SE gate * t2 + shortcut;  colstat_finish / seg_mean_std: the two finish passes of a statistic
 * reads / writes   space-separated tensors "buffer[col0:col1]:form"; buffers x0 r t2 xcat h s0 s1 a1 e xs xcs x0s rs (activation rows),
 *         semean seh gate stats gbias pooled (per segment), wpk (the fused chain's weights), feats, emb; a1 aliases x0 and e aliases xcat; forms f32 f16 split (SD_DT_SPLIT16)
 *         stat (a conv epilogue's per-tile column sums, parked in a dead buffer) scratch */
size_t sd_ecapa_plan_read(const sd_ecapa_weights* w, int B, int T, int M, int map_kind, char* buf, size_t cap);

/* What a conv entry would launch for these arguments (csrc/sd_conv_choice.h), without touching a device and
 * without dereferencing any pointer of *a: a test may pass any 16-byte aligned non-null addresses.  `op` names the entry: */
#define SD_CONV_OP_F32 0            /* sd_conv1d_cl_f32 */
#define SD_CONV_OP_F32_SYMMETRIC 1  /* the affinity's symmetric product (x == w) */
#define SD_CONV_OP_F32_STAT_ROWS 2  /* sd_conv1d_cl_f32 for a caller that takes column statistics in units of stat_rows rows (the ECAPA forward) */
#define SD_CONV_OP_F16 3            /* sd_conv1d_cl_f16 */
#define SD_CONV_OP_SPLIT16 4        /* sd_conv1d_cl_split16 */
#define SD_CONV_OP_PACKED 5         /* sd_conv1d_cl_packed_f32 (any span table) */
#define SD_CONV_OP_SEG_GEMM 6       /* sd_seg_gemm_f32 with an aligned scratch of scratch_bytes (0: none) */
/* One line per launch (sd_seg_gemm_f32: one or two):
 *     label \t grid \t block \t lds_bytes \t stat_rows
 * The same check and the same choice as the launching entry makes, with the sd_set_tuning values and experiment switches as a call
 * would read them now and a device of n_cu compute units (the MI355X: 256; 0: unknown).  Buffer and return convention of
 * sd_launch_log_read; 0, with sd_last_error() set, where the entry itself would refuse the arguments. */
size_t sd_conv_choice_read(const sd_conv_args* a, int op, int n_cu, size_t scratch_bytes, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_TRACE_H */
