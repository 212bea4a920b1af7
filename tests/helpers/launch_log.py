"""Which kernel ran: the launch log of libsd_hip.so (include/sd_hip_trace.h) as two context managers for the GPU tests.

A LABEL is the kernel's name, then <...> for the template instantiation and /... for the tile walk wherever the host chose one at run
time ("conv_gemm_f32_s64_kernel<32>", "conv_gemm_f16_t256_kernel<f16,direct>/lockstep").  `kernel_of(label)` is the name alone.

The labels a test expects are those of the MI355X (256 CUs: the lockstep walk of the 256x256 f16 kernel needs exactly that many)
under the shipped tuning defaults, or under the `sd_set_tuning` pins the test sets itself.  The log is host-side bookkeeping: it
neither synchronises nor touches the device, so a scope may hold any number of asynchronous launches.

Imported as a helper (tests/helpers on sys.path), like kernel_selection.py."""
import contextlib
import re

# the kernels of the three conv operators (sd_conv1d_cl_f32 and sd_seg_gemm_f32 / sd_conv1d_cl_packed_f32; sd_conv1d_cl_f16;
# sd_conv1d_cl_split16), as families for `expect_launches(exactly=..., family=...)`
F32_CONV = frozenset({"conv_gemm_f32_kernel", "conv_gemm_f32_s64_kernel", "skinny_gemm_f32_kernel", "conv_gemm_f32_vh_kernel",
                      "conv_gemm_f32_n64_kernel", "conv_gemm_f32_t256_kernel", "conv_gemm_f32_packed_kernel",
                      "seg_gemm_partial_f32_kernel", "seg_gemm_reduce_f32_kernel"})
F16_CONV = frozenset({"conv_gemm_f16_kernel", "conv_gemm_f16_t256_kernel", "conv_gemm_f16_w4_kernel"})
SPLIT_CONV = frozenset({"conv_gemm_split16_n128_kernel", "conv_gemm_f16_t256_kernel", "conv_gemm_f16_w4_kernel", "split16_pack_kernel"})
CONV = F32_CONV | F16_CONV | SPLIT_CONV


def kernel_of(label):
    """The __global__ function a label names: the text before the first '<' or '/'."""
    return re.split(r"[</]", label, maxsplit=1)[0]


@contextlib.contextmanager
def launches():
    """Count the launches of the scope: yields a dict that holds {label: count} once the scope is left.  Scopes do not nest."""
    from speech_diarization_amd import _native as N
    was_on = N.launch_log_enable(True)
    log = {}
    try:
        assert not was_on, "launch-log scopes do not nest"
        yield log
    finally:
        log.update(N.launch_log_read())
        N.launch_log_enable(False)


@contextlib.contextmanager
def expect_launches(exactly=(), at_least=(), family=None):
    """Every label of `exactly` and of `at_least` must have been launched inside the scope.  Beyond that, no label whose kernel
    belongs to `family` (a set of kernel names; default: the kernels that `exactly` names) may have run unless `exactly` lists it.
    Labels outside the family (helper launches such as l2norm or fill) are not looked at."""
    exactly, at_least = frozenset(exactly), frozenset(at_least)
    family = frozenset(kernel_of(lb) for lb in exactly) if family is None else frozenset(family)
    with launches() as log:
        yield log
    missing = sorted(lb for lb in exactly | at_least if not log.get(lb))
    assert not missing, f"not launched: {missing}; launched: {sorted(log)}"
    other = sorted(lb for lb in log if kernel_of(lb) in family and lb not in exactly | at_least)
    assert not other, f"launched besides {sorted(exactly | at_least)}: {other}"
