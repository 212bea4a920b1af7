"""No-GPU checks of the conv operators' choice layer (csrc/sd_conv_choice.h) through `sd_conv_choice_read`
(include/sd_hip_trace.h): which kernel, grid and LDS size an entry would launch is a pure function of the shape, the alignments, the
caller's flags and the tuning, so every rule is checked here, at every shape, and not only where a GPU test happens to launch.

The references are independent statements of the rules: `kernel_selection.f32_conv_label` (the f32 rules restated in Python) and the
hand-derived labels of tests/helpers/exact_cases.py, which the GPU tests hold the launch log to."""
import itertools
import os
import re
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import conv_choice as CC  # noqa: E402
import exact_cases as E  # noqa: E402
from kernel_selection import CONV_KERNELS, f32_conv_label, restore_conv_kernel, select_conv_kernel  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.skipif(not N.LIB_PATH.exists(), reason="libsd_hip.so is not built")
CSRC = N.PKG_DIR / "csrc"
MI355X = 256        # CUs


def _read(a, op, n_cu=MI355X, scratch=0):
    lines = N.conv_choice_read(a, op, n_cu, scratch)
    for ln in lines:
        CC.check_line(ln, a, op)
    return lines


def _labels(a, op, **kw):
    return tuple(ln[0] for ln in _read(a, op, **kw))


@pytest.fixture
def tuning():
    yield
    restore_conv_kernel()
    for key in (N.SD_TUNE_F16_NARROW_TILES, N.SD_TUNE_T256_LOCKSTEP_TILES):
        N.check(N.load().sd_set_tuning(key, -1), "sd_set_tuning")


# ------------------------------------------------------------------ the f32 rules, densely

SWEEP_T = (1, 5, 64, 79, 80, 96, 112, 127, 128, 131, 201)
SWEEP_COUT = (8, 40, 64, 128, 192, 256, 1016, 1024, 1536, 3072)
SWEEP_ROWS = (32, 64, 128, 300, 1000, 4000, 9000, 16500, 33000, 70000)     # M ~ these: one 32-row tile .. past 1024 tiles of 256x256 at cout 1024


def test_f32_choice_equals_the_python_statement_over_the_dense_sweep(tuning):
    """Every selection x T x cout x M x (colstat, tee_add, a caller that takes stat_rows): wherever the entry accepts the arguments, its
    label is f32_conv_label's.  A colstat is refused below T = 64, off cout % 256 and with a tee; nothing else of the sweep is."""
    seen, refused = set(), 0
    for sel in CONV_KERNELS:
        select_conv_kernel(sel)
        for T, cout, rows in itertools.product(SWEEP_T, SWEEP_COUT, SWEEP_ROWS):
            M = max(1, -(-rows // T)) * T
            for colstat, tee_add, stat_rows in itertools.product((False, True), repeat=3):
                a = CC.conv_args(M, T, 64, cout, tee=(0, 8) if tee_add else None, tee_add=tee_add, colstat=colstat)
                try:
                    (label,) = _labels(a, "f32_stat_rows" if stat_rows else "f32")
                except N.SdError:
                    assert colstat and (T < 64 or cout % 256 or tee_add), (sel, M, T, cout, colstat, tee_add, N.last_error())
                    refused += 1
                    continue
                assert label == f32_conv_label(sel, M, T, cout, colstat, tee_add, stat_rows), (sel, M, T, cout, colstat, tee_add, stat_rows)
                seen.add(label)
    assert refused and seen == set(E._selections("").values()) - {""} | {E._S32, E._S64, E._SK, E._T256}, sorted(seen)
    assert max(SWEEP_ROWS) // 256 * 4 > 1024       # the sweep passes 1024 tiles of 256x256 at cout 1024


# ------------------------------------------------------------------ the hand-derived labels of exact_cases.py

F32_CASES = [n for n in E.CONV_CASE_NAMES if n[0] == "S"] + ["C3x128-256", "C5x64-256"]
F16_CASES = [n for n in E.CONV_CASE_NAMES if n[0] == "H"] + ["C3x128-256", "C5x64-256", "C11x64-1024", "C3x128-1024"]
SPLIT_CASES = [n for n in E.CONV_CASE_NAMES if n[0] in "NW"]


def test_f32_seg_gemm_and_packed_labels_are_the_hand_derived_ones(tuning):
    lib = N.load()
    for name in F32_CASES:
        shape = name if name[0] == "C" else name.split("-")[0]
        for sel in CONV_KERNELS:
            select_conv_kernel(sel)
            assert _labels(CC.case_args(name, "f32"), "f32") == (E.F32_LABELS[shape][sel],), (name, sel)
    restore_conv_kernel()
    for name in (n for n in F32_CASES if n.startswith("S4")):
        a = CC.case_args(name, "seg")
        need = int(lib.sd_seg_gemm_scratch_bytes(a.M, a.cin_pad, a.cout))
        assert need > 0 and _labels(a, "seg_gemm", scratch=need) == E.SEG_GEMM_LABELS
        # without the scratch, or with too little of it, the layer takes the plain operator's choice
        assert _labels(a, "seg_gemm", scratch=need - 4) == _labels(a, "seg_gemm") == _labels(a, "f32") == (E.F32_LABELS["S4"]["auto"],)
    for name in ("P-rows", "P-chan", "P-dense"):
        assert _labels(CC.case_args(name, "packed"), "packed") == (E.PACKED_LABEL,)


def test_f16_and_split16_labels_are_the_hand_derived_ones(tuning):
    """Both f16_tiles settings, every dtype pair, both lockstep settings; and a device that has not 256 CUs never walks in lockstep."""
    lib = N.load()
    lockstep_seen = 0
    for tiles, lockstep in itertools.product(("auto", "wide256"), (False, True)):
        N.check(lib.sd_set_tuning(N.SD_TUNE_F16_NARROW_TILES, 0 if tiles == "wide256" else -1), "sd_set_tuning")
        N.check(lib.sd_set_tuning(N.SD_TUNE_T256_LOCKSTEP_TILES, 0 if lockstep else -1), "sd_set_tuning")
        for name, x16, y16 in itertools.product(F16_CASES, (True, False), (True, False)):
            a = CC.case_args(name, "f16", x16, y16)
            got = _labels(a, "f16")
            assert got == (E.f16_label(name, tiles, x16, y16, lockstep),), (name, tiles, x16, y16, lockstep)
            lockstep_seen += got[0].endswith("/lockstep")
            assert not any("/lockstep" in lb for n_cu in (0, 64, 304) for lb in _labels(a, "f16", n_cu=n_cu))
        for name, split_out in itertools.product(SPLIT_CASES, (False, True)):
            if split_out and E._cout(name) % 32:
                continue
            a = CC.case_args(name, "narrow" if name[0] == "N" else "wide", split_out=split_out)
            want = tuple(lb for lb in E.split_labels(name, split_out, lockstep) if lb != "split16_pack_kernel")       # (the pack pass is an entry of its own)
            got = _labels(a, "split16")
            assert got == want, (name, split_out, lockstep)
            lockstep_seen += got[0].endswith("/lockstep")
            assert not any("/lockstep" in lb for lb in _labels(a, "split16", n_cu=0))
    assert lockstep_seen >= 4


def test_refusals_are_the_entries_own(tuning):
    """0 with sd_last_error() set where the entry itself would refuse: a wrong dtype, a misaligned slice, tee_add on the wide split
    form, an unknown op; and the short-buffer convention of sd_launch_log_read."""
    import ctypes as C
    lib = N.load()
    for a, op, why in ((CC.conv_args(64, 64, 64, 64, w=CC.F16), "f32", "w_dtype"), (CC.conv_args(64, 64, 62, 64), "f32", "multiple of 4"),
                       (CC.conv_args(64, 64, 64, 64, x=CC.SPLIT, w=CC.SPLIT, tee=(0, 8), tee_add=True), "split16", "tee_add"),
                       (CC.conv_args(64, 3, 64, 64, taps=7), "f16", "w_dtype"), (CC.conv_args(64, 1, 64, 64, taps=3, w=CC.F16), "f16", "reflect"),
                       (CC.conv_args(64, 64, 64, 64, colstat=True), "packed", "no column statistics")):
        with pytest.raises(N.SdError, match=why):
            N.conv_choice_read(a, op)
    assert int(lib.sd_conv_choice_read(C.byref(CC.conv_args(64, 64, 64, 64)), 7, 256, 0, None, 0)) == 0 and "unknown op" in N.last_error()
    a = CC.conv_args(171, 57, 36, 72)
    text = b"conv_gemm_f32_s64_kernel<32>\t12\t256\t65536\t128\n"
    buf = C.create_string_buffer(b"x" * 64, 64)
    assert int(lib.sd_conv_choice_read(C.byref(a), 0, 256, 0, buf, 64)) == len(text) + 1 and buf.value == text
    assert int(lib.sd_conv_choice_read(C.byref(a), 0, 256, 0, None, 0)) == len(text) + 1
    small = C.create_string_buffer(b"xxxxxx", 6)
    assert int(lib.sd_conv_choice_read(C.byref(a), 0, 256, 0, small, 4)) == len(text) + 1 and small.raw == b"con\0xx"


# ------------------------------------------------------------------ one statement; nothing left of the removed switches

REMOVED = ("SD_SKINNY_TILES", "SD_S64_TILES", "SD_F32_N64", "SD_F32_TILE_ROWS", "SD_F32_WIDE", "SD_PERSIST", "SD_TILE_ORDER", "SD_S64_HALF",
           "SD_SEG_SPLITK", "SD_F32_DMA", "SD_F16_W4", "SD_WITH_W4")


def _code(text):
    return re.sub(r"//[^\n]*", "", text)


def test_each_rule_is_stated_once():
    files = {f.name: f.read_text() for f in sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.h"))}
    code = {name: _code(text) for name, text in files.items()}
    where = lambda pattern: [name for name, text in code.items() for _ in re.finditer(pattern, text)]  # noqa: E731
    assert where(r"cout <= 1024") == ["sd_conv_choice.h"]                               # wide_goes_narrow's expression
    assert where(r"<= 56\b") == ["sd_ecapa.hip"]                                         # the 56-tile rule of the narrow route
    header = code["sd_conv_choice.h"]
    defaults = re.search(r"constexpr long sd_tune_default\(.*?\n}", header, flags=re.S).group(0)
    for literal in ("128L", "1024L"):      # the SD_TUNE defaults: in sd_tune_default and nowhere else (the lockstep rule's 4L * 256 is no default)
        assert where(rf"\b{literal}\b") == ["sd_conv_choice.h"] * defaults.count(literal) and defaults.count(literal) >= 1, literal
    setter = re.search(r"int sd_set_tuning\(.*?\n}", code["sd_conv_gemm.hip"], flags=re.S).group(0)
    assert "sd_tune_stored(key, value)" in setter and not re.search(r"\b\d{2,}", setter)
    for name in REMOVED:
        assert not [f for f, text in files.items() if re.search(rf"\b{name}\b", text)], name
    envs = set(re.findall(r'sd_experiment_env\("(SD_[A-Z0-9_]+)"\)', "".join(files.values())))
    assert {"SD_F16_KERNEL", "SD_T256_DIRECT"} <= envs and not envs & set(REMOVED)
    # the choice header is host-only C++: no HIP header, no environment, no atomic, no launch
    raw = files["sd_conv_choice.h"]
    assert re.findall(r'#include [<"]([^>"]+)[>"]', raw) == ["stddef.h", "sd_hip.h"]
    assert not re.search(r"getenv|std::atomic|hipLaunch|hipGet|hipDevice|<<<", header)


def test_the_choice_compiles_and_runs_alone_under_the_sanitizers(tmp_path):
    """tests/helpers/conv_choice_pure.cpp: sd_conv_choice.h in a plain C++ program with its own main, address + undefined-behaviour
    sanitizers, nothing preloaded; every sd_choose_* over the sweep's corners up to M = 2^31 - 1 and down to cout = 1."""
    cxx = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(cxx), "no clang++ on this machine"
    exe = tmp_path / "conv_choice_pure"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           f"-I{N.PKG_DIR.parent / 'include'}", os.path.join(HERE, "helpers", "conv_choice_pure.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0 and not ran.stderr, (ran.returncode, ran.stderr[-2000:])
    assert int(ran.stdout.split()[0]) > 1_000_000
