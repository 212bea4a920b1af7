"""No-GPU checks of the launch log (include/sd_hip_trace.h) and of the census of launch labels (tests/helpers/kernel_census.py): the
binding table, the untouched main ABI, the log with nothing launched, and -- read out of the source text of csrc/*.hip and of the
conv operators' label table in csrc/sd_conv_choice.h -- that every kernel has a label, every label a GPU test that asserts it ran,
and every exemption the guard it claims."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import kernel_census as K  # noqa: E402
import launch_log as L  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402

needs_lib = pytest.mark.skipif(not N.LIB_PATH.exists(), reason="libsd_hip.so is not built")
CSRC = N.PKG_DIR / "csrc"
LABEL = re.compile(r'"([a-z0-9_]+_kernel(?:<[^">]*>)?(?:/[a-z]+)?)"')


# ------------------------------------------------------------------ ABI

@needs_lib
def test_header_and_binding_table_name_the_same_exported_entries():
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_trace.h").read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = set(re.findall(r"\b(sd_[a-z0-9_]+)\s*\(", header))
    assert names == set(N.TRACE_PROTOTYPES) == {"sd_trace_abi_version", "sd_launch_log_enable", "sd_launch_log_read", "sd_ecapa_plan_read",
                                                    "sd_conv_choice_read"}
    assert not names & (set(N.PROTOTYPES) | set(N.SPECTRAL_PROTOTYPES) | set(N.AHC_PROTOTYPES) | set(N.HDBSCAN_PROTOTYPES))
    lib = N.load()
    for name, (res, args) in N.TRACE_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    assert names <= set(re.findall(r"\bT (sd_[a-z0-9_]+)$", out, flags=re.M))


@needs_lib
def test_versions_and_struct_sizes_are_untouched():
    lib = N.load()
    assert lib.sd_trace_abi_version() == 3 == N.SD_TRACE_ABI_VERSION
    assert lib.sd_abi_version() == 11 and lib.sd_spectral_abi_version() == 1 and lib.sd_ahc_abi_version() == 1 and lib.sd_hdbscan_abi_version() == 1
    assert [int(lib.sd_sizeof(i)) for i in range(5)] == [184, 88, 1672, 13944, 0]       # the committed layouts of ABI 11
    header = open(N.PKG_DIR.parent / "include" / "sd_hip.h").read()
    assert re.search(r"#define\s+SD_ABI_VERSION\s+11\b", header)


# ------------------------------------------------------------------ the log with nothing launched

@needs_lib
def test_enable_read_and_disable_without_a_launch():
    lib = N.load()
    assert N.launch_log_enable(False) is False                       # off by default
    assert N.launch_log_enable(True) is False and N.launch_log_enable(True) is True     # returns the previous state
    assert N.launch_log_read() == {}
    assert int(lib.sd_launch_log_read(None, 0)) == 1                 # the empty text: its NUL alone
    buf = C.create_string_buffer(b"x" * 8, 8)
    assert int(lib.sd_launch_log_read(buf, 8)) == 1 and buf.raw[0] == 0 and buf.raw[1:] == b"x" * 7
    assert N.launch_log_enable(False) is True and N.launch_log_enable(False) is False
    assert N.launch_log_read() == {}
    with L.launches() as log:
        pass
    assert log == {}
    with pytest.raises(AssertionError, match="not launched"):
        with L.expect_launches(exactly=["conv_gemm_f32_kernel<dma>"]):
            pass
    assert N.launch_log_enable(False) is False                       # a failed expectation leaves the log off


def test_expectations_are_judged_by_family():
    assert L.kernel_of("conv_gemm_f16_t256_kernel<f16,direct>/lockstep") == "conv_gemm_f16_t256_kernel"
    assert L.kernel_of("skinny_gemm_f32_kernel") == "skinny_gemm_f32_kernel" and L.kernel_of("affinity_sym_kernel<exact f32>") == "affinity_sym_kernel"
    assert L.F32_CONV | L.F16_CONV | L.SPLIT_CONV == L.CONV


# ------------------------------------------------------------------ the census, from the source text

def _sources():
    """The .hip files, and the header that holds the conv operators' label table (the operators hand `choice.label` to the log)."""
    return {f.name: f.read_text() for f in sorted(CSRC.glob("*.hip")) + [CSRC / "sd_conv_choice.h"]}


def _labels():
    return {lb for text in _sources().values() for lb in LABEL.findall(text)}


def test_every_kernel_has_a_label():
    text = "".join(_sources().values())
    kernels = set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", text))
    assert len(kernels) >= 50 and all(k.endswith("_kernel") for k in kernels), sorted(kernels)
    named = {L.kernel_of(lb) for lb in _labels()}
    assert kernels == named, (sorted(kernels - named), sorted(named - kernels))
    # every label is handed to the log: it stands in an SD_CHECK_LAUNCH or in a table / function such a call reads.  The conv operators
    # have one SD_CHECK_LAUNCH(c.label) per file, behind the switch over the ids of sd_conv_label's table: every id of the table is a case
    assert len(re.findall(r"\bSD_CHECK_LAUNCH\(", text)) == 39        # (43 until each fbank launch was written once: one site serves both instantiations)
    assert len(re.findall(r"\bSD_CHECK_LAUNCH\(c\.label\)", text)) == 2
    table = _function_text_c(_sources()["sd_conv_choice.h"], "sd_conv_label")
    ids = set(re.findall(r"case (SD_K_[A-Z0-9_]+):", table)) | {"SD_K_SPLIT_N128"}          # (the table's default)
    assert len(ids) == 24 and len(LABEL.findall(table)) == 27
    cases = set(re.findall(r"case (SD_K_[A-Z0-9_]+):", "".join(t for n, t in _sources().items() if n.endswith(".hip"))))
    assert cases == ids, (sorted(ids - cases), sorted(cases - ids))


def _function_text_c(text, fn):
    """The body of the C++ function `fn`: from its name to the first line that is a lone closing brace."""
    return re.search(rf"\b{fn}\(.*?^}}", text, flags=re.M | re.S).group(0)


def test_the_census_table_equals_the_labels_of_the_sources():
    labels = _labels()
    assert labels == set(K.KERNEL_TESTS), (sorted(labels - set(K.KERNEL_TESTS)), sorted(set(K.KERNEL_TESTS) - labels))
    assert {lb for lb, t in K.KERNEL_TESTS.items() if t is None} == set(K.EXEMPT)


# helpers of the GPU modules that build a label for the kernel named (tests/helpers/exact_cases.py states the labels they return, or the
# helper's own text holds the kernel's name): a test may name its kernel through one of them instead of spelling it
PRODUCERS = {
    **{k: ("F32_LABELS", "SEG_GEMM_LABELS", "PACKED_LABEL") for k in L.F32_CONV},
    "conv_gemm_f16_kernel": ("f16_label",), "conv_gemm_f16_t256_kernel": ("f16_label", "split_labels"),
    "conv_gemm_split16_n128_kernel": ("split_labels",), "split16_pack_kernel": ("split_labels",),
    "colstat_finish_kernel": ("_check_colstat",), "asp_pool_kernel": ("_asp_pool",), "asp_pool_lds_kernel": ("_asp_pool",),
    "asp_attend_pool_f32_kernel": ("_attend",), "asp_attend_pool_f16_kernel": ("_attend",),
    "affinity_sym_kernel": ("_affinity_labels",), "fill_f32_kernel": ("_affinity_labels",), "conv_gemm_f32_kernel": ("F32_LABELS", "_affinity_labels"),
    "hdb_core_kernel": ("_core_labels",), "hdb_core_finish_kernel": ("_core_labels",),
}


def _function_text(text, fn):
    """The source of top-level function `fn`: from its def to the next line that starts a top-level statement."""
    m = re.search(rf"^def {fn}\(.*?(?=^\S)", text + "\nend", flags=re.M | re.S)
    return m.group(0) if m else None


def test_every_named_test_exists_and_asserts_its_label():
    """The named function exists in a GPU module, runs under expect_launches, and names the label's kernel: in its own text, or through
    a helper of PRODUCERS whose text (in the module or in exact_cases.py) holds the kernel's name."""
    cases = open(os.path.join(HERE, "helpers", "exact_cases.py")).read()
    for label, test in K.KERNEL_TESTS.items():
        if test is None:
            continue
        module, fn = test
        text = open(os.path.join(HERE, module + ".py")).read()
        body = _function_text(text, fn)
        assert body, (label, module, fn)
        assert "pytestmark = pytest.mark.gpu" in text, module
        kernel = L.kernel_of(label)
        helpers = [h for h in PRODUCERS.get(kernel, ()) if re.search(rf"\b{h}\b", body)]
        assert "expect_launches" in body or any("expect_launches" in (_function_text(text, h) or "") for h in helpers), (label, fn)
        if kernel in body:
            continue
        assert helpers, f"{module}::{fn} never names {kernel}"
        assert any(kernel in (_function_text(text, h) or "") or (h in cases and kernel in cases) for h in helpers), (label, fn, helpers)
    # the rule bites: a test that never names the kernel is not accepted for it
    exact = open(os.path.join(HERE, "test_gpu_exact.py")).read()
    body = _function_text(exact, "test_viterbi_ties_go_to_the_first_state")
    assert "viterbi_kernel" in body and "topk_mean_std_kernel" not in body and not any(h in body for h in PRODUCERS)


def _check_exemption(label, reason, guard, sources):
    assert reason and guard.startswith(K.ALLOWED_GUARDS), label
    hits = [(name, i, text.splitlines()) for name, text in sources.items() for i, line in enumerate(text.splitlines()) if f'"{label}"' in line]
    assert hits, label
    for name, i, lines in hits:
        if guard.startswith("#ifdef"):
            open_ifs = []
            for line in lines[:i]:
                word = line.lstrip()
                if word.startswith(("#ifdef", "#ifndef", "#if ")):
                    open_ifs.append(word.split("//")[0].strip())
                elif word.startswith("#endif"):
                    open_ifs.pop()
            assert guard in open_ifs, f"{label}: {guard} is not open at {name}:{i + 1} ({open_ifs})"
        else:
            assert any(guard in line for line in lines[max(0, i - 60):i + 1]), f"{label}: no {guard} within 60 lines above {name}:{i + 1}"


def test_every_exemption_stands_behind_its_guard():
    """The guard must be one of the kinds the shipped build never passes and must stand in the label's own file: an #ifdef still
    open at every launch site that names the label, or an experiment variable read at most 60 lines above it.  No label is exempt
    today, so the rule is shown on a synthetic source: it accepts both kinds of guard and bites on each."""
    for label, (reason, guard) in K.EXEMPT.items():
        _check_exemption(label, reason, guard, _sources())
    assert K.EXEMPT == {}        # every label of the sources is reachable in the shipped build
    env = 'sd_experiment_env("SD_TOY")'
    toy = {"toy.hip": "\n".join(['static const bool on = [] { return ' + env + ' != nullptr; }();', 'if (on) SD_CHECK_LAUNCH("toy_a_kernel");'] + ["//"] * 60 +
                                ['SD_CHECK_LAUNCH("toy_b_kernel");', "#ifdef SD_STAMP", 'SD_CHECK_LAUNCH("toy_c_kernel");', "#endif",
                                 'SD_CHECK_LAUNCH("toy_d_kernel");'])}
    _check_exemption("toy_a_kernel", "behind the variable", env, toy)
    _check_exemption("toy_c_kernel", "stamp builds only", "#ifdef SD_STAMP", toy)
    for label, guard, why in (("toy_b_kernel", env, "no .* within 60 lines"), ("toy_d_kernel", "#ifdef SD_STAMP", "is not open"),
                              ("toy_a_kernel", "#ifdef SD_OTHER", "toy_a_kernel"), ("toy_e_kernel", env, "toy_e_kernel")):
        with pytest.raises(AssertionError, match=why):
            _check_exemption(label, "a reason", guard, toy)

