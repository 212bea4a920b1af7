/*
 * sd_hip_trace.h — the launch log of libsd_hip.so (same shared object as sd_hip.h, a binding table of its own:
 * `_native.TRACE_PROTOTYPES`, version `sd_trace_abi_version()`).
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

#ifdef __cplusplus
extern "C" {
#endif

#define SD_TRACE_ABI_VERSION 1

int sd_trace_abi_version(void);

/* on != 0: clear the counts and start counting; on == 0: stop (the counts stay readable).  Returns the previous state (0 / 1). */
int sd_launch_log_enable(int on);

/* The counts since the last sd_launch_log_enable(1) as lines "label\tcount\n", sorted by label, NUL-terminated.  At most cap bytes are
 * written (a truncated text is still terminated; buf may be NULL with cap 0).  Returns the bytes the whole text needs, its NUL
 * included: a result above cap says the buffer was short. */
size_t sd_launch_log_read(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SD_HIP_TRACE_H */
