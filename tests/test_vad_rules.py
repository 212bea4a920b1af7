"""No-GPU checks of the device VAD (include/sd_hip_vad.h: sd_vad_energy_grouped_f32, sd_vad_segments_grouped,
speech-diarization_amd/csrc/vad/, vad_gpu.py, vad="device"): the numpy statement of both entries (tests/helpers/vad_ref.py) against
scipy.ndimage exhaustively and against vad.py, the capacity bound, the host tail against `mask_to_segments`, the header and its
binding table, the census of the new source directory, the pure check (csrc/vad/sd_vad_check.h, built alone with sanitizers) with its
codes and precedence, the workspace formula, the band condition on the inputs of the GPU end-to-end tests, and the opt-in routes."""
import inspect
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import launch_log as L  # noqa: E402
import vad_ref as V  # noqa: E402
from abi_rules import ARG, WS, check_header_and_table, check_versions, refused  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import diarization_baseline as db  # noqa: E402
from speech_diarization_amd import ops, synth, vad, vad_gpu  # noqa: E402

CSRC = N.PKG_DIR / "csrc"
NAMES = {"sd_vad_abi_version", "sd_vad_energy_grouped_f32", "sd_vad_segments_workspace_bytes", "sd_vad_segments_grouped"}
KERNELS = {"vad_energy_kernel", "vad_segments_kernel"}


# ------------------------------------------------------------------ the statement against scipy and vad.py

def test_the_run_form_of_the_morphology_equals_scipy_exhaustively():
    """Every mask of at most 12 frames, every line length in use: opening keeps the runs of at least L; closing joins runs less than L
    apart and clears the first L // 2 and the last L - 1 - L // 2 frames"""
    checked = 0
    for n in range(1, 13):
        for bits in itertools.product((False, True), repeat=n):
            m = np.array(bits)
            runs = V.runs_of(m)
            assert np.array_equal(V.mask_of(runs, n), m)
            for ln in V.LINES:
                line = np.ones(ln, bool)
                assert np.array_equal(V.mask_of(V.opening(runs, ln), n), ndimage.binary_opening(m, structure=line)), (bits, ln)
                assert np.array_equal(V.mask_of(V.closing(runs, ln, n), n), ndimage.binary_closing(m, structure=line)), (bits, ln)
                checked += 1
    assert checked == 7 * (2 ** 13 - 2)


def test_the_capacity_bound_holds_exhaustively():
    """A mask of n frames has at most (n + 1) // 2 runs (every mask of at most 16 frames), and no stage makes more (every mask of at
    most 12 frames, every parameter set): the share of seg_start / seg_end the header asks for"""
    for n in range(1, 17):
        m = np.arange(2 ** n, dtype=np.int64)
        starts = m & ~(m << 1)                           # a run starts where a bit is set and the one below it is not
        runs = sum((starts >> b) & 1 for b in range(n))
        assert runs.max() == (n + 1) // 2 == vad_gpu.run_capacity(n)
    for n in range(1, 13):
        for bits in itertools.product((0.1, 0.9), repeat=n):
            for prm in V.PARAMS.values():
                counts = [len(r) for r in V.stages(np.array(bits, np.float32), 0.6, 0.4, *prm)]
                assert counts[0] <= (n + 1) // 2 and all(b <= a for a, b in zip(counts, counts[1:])), (bits, prm)


def _host_chain(p, hop_ms, on=0.6, off=0.4, open_ms=80.0, close_ms=40.0, min_speech_ms=250.0, min_gap_ms=100.0, pad_ms=80.0):
    mask = vad.morph_open_close(vad.hysteresis_binarize(p, on, off), hop_ms, open_ms, close_ms)
    return mask, vad.mask_to_segments(mask, hop_ms, min_speech_ms, min_gap_ms, pad_ms)


@pytest.mark.parametrize("hop_ms", (10.0, 12.5))
def test_the_statement_and_the_driver_equal_vad_py(hop_ms):
    """Random and constructed probabilities through `vad_gpu.segments_from_probs_groups` with the statement as its launch: the masks
    of `morph_open_close(hysteresis_binarize(.))` and the lists of `mask_to_segments`, both rounding regimes included"""
    rs = np.random.RandomState(int(hop_ms))
    recs = []
    for n in (1, 2, 5, 37, 361, 400, 1000):
        recs += list(V.prob_families(n, seed=n).values())
    recs += [V.built_probs([rs.randint(1, 50) for _ in range(40)], lead=rs.randint(0, 9), tail=rs.randint(0, 9)) for _ in range(20)]
    recs.append(np.full(361, 0.9, np.float32))           # speech to the last frame of 361: the clamp's Python rounding at hop 12.5
    ff = np.concatenate([[0], np.cumsum([len(p) for p in recs])])
    for kw in ({}, dict(open_ms=50.0, close_ms=0.0, min_speech_ms=350.0, pad_ms=40.0), dict(open_ms=0.0, close_ms=90.0, min_gap_ms=0.0, pad_ms=0.0),
               dict(on=0.7, off=0.2)):
        prm = dict(dict(on=0.6, off=0.4, open_ms=80.0, close_ms=40.0, min_speech_ms=250.0, min_gap_ms=100.0, pad_ms=80.0), **kw)
        segs, masks = vad_gpu.segments_from_probs_groups(np.concatenate(recs), ff, hop_ms, prm["on"], prm["off"], prm["open_ms"], prm["close_ms"],
                                                         prm["min_speech_ms"], prm["min_gap_ms"], prm["pad_ms"], return_mask=True,
                                                         launch=V.segments_launch)
        some = 0
        for p, seg, mask in zip(recs, segs, masks):
            want_mask, want = _host_chain(p, hop_ms, **prm)
            assert np.array_equal(mask, want_mask) and seg == want
            some += len(want)
        assert some > 100
    for p in recs[:30]:
        assert np.array_equal(V.hysteresis(p, 0.6, 0.4), V.hysteresis_literal(p, 0.6, 0.4))
        assert np.array_equal(V.hysteresis(p, 0.6, 0.4), vad.hysteresis_binarize(p, 0.6, 0.4))


def test_the_host_tail_equals_mask_to_segments():
    """`vad_gpu.runs_to_segments` restates the padding, the clamp and the rounding of `mask_to_segments`: equal on every run list"""
    rs = np.random.RandomState(1)
    for hop_ms, pad_ms in ((10.0, 40.0), (12.5, 80.0), (12.5, 30.0), (10.0, 0.0), (16.0, 100.0)):
        for _ in range(150):
            n = rs.randint(1, 500)
            mask = np.repeat(rs.uniform(0, 1, n // 4 + 1) < 0.5, 4)[:n]
            runs = V.runs_of(mask)
            want = vad.mask_to_segments(mask, hop_ms, 0.0, 0.0, pad_ms)
            assert vad_gpu.runs_to_segments([s for s, _ in runs], [e for _, e in runs], n, hop_ms, pad_ms) == want
    assert vad_gpu.runs_to_segments([], [], 10, 10.0) == []
    assert vad_gpu.runs_to_segments([0], [361], 361, 12.5, 0.0) == [(0.0, 4.512)]                # numpy's rounding: no clamp
    assert vad_gpu.runs_to_segments([0], [361], 361, 12.5, 40.0) == [(0.0, 4.513)]               # the clamp: Python's
    assert (vad_gpu.line_lengths(10.0, 80.0, 40.0), vad_gpu.line_lengths(12.5, 80.0, 40.0), vad_gpu.line_lengths(10.0, 0.0, -1.0)) == \
        ((8, 4), (6, 3), (1, 1))


def test_the_energy_statement_is_the_host_scorer_in_float64():
    rs = np.random.RandomState(2)
    y = (0.05 * rs.standard_normal(16000) * (np.arange(16000) % 4000 < 2500)).astype(np.float32)
    for (win_ms, hop_ms), scorer in (((30.0, 10.0), vad.EnergyScorer()), ((25.0, 12.5), vad.EnergyScorer(-30.0, 0.9))):
        win, hop = vad_gpu.frame_sizes(16000, win_ms, hop_ms)
        host = vad.SileroVAD(model=scorer).probs(y, 16000, win_ms, hop_ms)
        p64 = V.energy_probs64(y, win, hop, scorer.threshold_db, scorer.slope)
        assert host.shape == p64.shape == (V.frame_count(len(y), win, hop),) and np.abs(host - p64).max() < 1e-5
    assert np.abs(V.energy_probs64(np.zeros(480, np.float32), 480, 160) - 1 / (1 + np.exp(0.6 * 85.0))).max() < 1e-30
    y[5000] = np.nan
    p = V.energy_probs64(y, 480, 160)
    assert np.array_equal(np.flatnonzero(np.isnan(p)), [t for t in range(len(p)) if t * 160 <= 5000 < t * 160 + 480])
    # the refusals of frame_audio, word for word
    for n in (0, 479):
        with pytest.raises(ValueError) as theirs:
            vad.frame_audio(np.zeros(n, np.float32), 16000)
        with pytest.raises(ValueError) as ours:
            vad_gpu.frame_counts([480, n], 480, 160)
        assert str(ours.value) == str(theirs.value)
    with pytest.raises(ValueError, match="Invalid hop_length: 0"):
        vad_gpu.frame_sizes(16000, 30.0, 0.01)
    assert vad_gpu.frame_counts([480, 639, 640], 480, 160).tolist() == [1, 1, 2]


def test_the_inputs_of_the_gpu_end_to_end_tests_are_band_clean():
    """No float64 probability of any signal the GPU end-to-end tests use lies within 1e-4 of a threshold (a condition on the inputs:
    an f32 scorer and the device's decide alike there; the bar of the energy test, a few 1e-6, stays below the band)"""
    signals = [V.bursty_signal(sec, seed) for sec, seed in V.E2E_SIGNALS] + [V.silent_signal(2.0), np.zeros(4000, np.float32)]
    signals += [synth.synthetic_conversation(12.0, 2, seed=0).wav.astype(np.float32), np.zeros(3 * 16000, np.float32),
                synth.synthetic_conversation(8.0, 3, seed=1).wav.astype(np.float32)]
    frames = 0
    for y in signals:
        p = V.energy_probs64(y, 480, 160)
        frames += len(p)
        assert V.band_clean(y), float(min(np.abs(p - 0.6).min(), np.abs(p - 0.4).min()))
    assert frames > 6000 and V.BAND == 1e-4
    text = open(os.path.join(HERE, "test_gpu_vad.py")).read()
    assert "V.E2E_SIGNALS" in text and "synthetic_conversation(12.0, 2, seed=0)" in text and "synthetic_conversation(8.0, 3, seed=1)" in text
    assert len(re.findall(r"synthetic_conversation\(|bursty_signal\(|silent_signal\(", text)) == 4


# ------------------------------------------------------------------ ABI

def test_header_and_binding_table_name_the_same_exported_entries():
    others = (N.PROTOTYPES, N.SPECTRAL_PROTOTYPES, N.AHC_PROTOTYPES, N.HDBSCAN_PROTOTYPES, N.DIAG_PROTOTYPES, N.TRACE_PROTOTYPES, N.TREE_ENTRIES,
              N.CUT_ENTRIES, N.KMEANS_ENTRIES)
    assert check_header_and_table("sd_hip_vad.h", N.VAD_ENTRIES, others) == NAMES
    assert ops._VAD_LAUNCHABLE == NAMES and not NAMES & (ops._LAUNCHABLE | ops._CUT_LAUNCHABLE | ops._KMEANS_LAUNCHABLE)
    assert '("sd_hip_vad.h", VAD_ENTRIES, "sd_vad_abi_version", SD_VAD_ABI_VERSION, "VAD ")' in open(N.__file__).read()
    with pytest.raises(ValueError, match="not an entry"):
        ops.launch("sd_vad_segments", torch.zeros(1))


def test_the_new_version_is_one_and_every_other_is_untouched():
    assert N.SD_VAD_ABI_VERSION == 1
    check_versions(sd_vad_abi_version=1, sd_kmeans_abi_version=1, sd_cut_abi_version=1, sd_tree_abi_version=1, sd_abi_version=11,
                   sd_spectral_abi_version=1, sd_ahc_abi_version=1, sd_hdbscan_abi_version=1, sd_diag_abi_version=1, sd_trace_abi_version=3)
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_vad.h").read()
    assert re.search(r"#define\s+SD_VAD_ABI_VERSION\s+1\b", header)
    for name, value in (("SHORT", V.SHORT), ("BAD_RANGE", V.BAD_RANGE), ("BAD_FRAMES", V.BAD_FRAMES), ("BAD_CAPACITY", V.BAD_CAPACITY),
                        ("BAD_PROMISE", V.BAD_PROMISE), ("LDS_FRAMES", V.LDS_FRAMES)):
        assert re.search(rf"#define\s+SD_VAD_{name}\s+{value}\b", header), name
    assert (vad_gpu.SHORT, vad_gpu.BAD_RANGE, vad_gpu.BAD_FRAMES, vad_gpu.BAD_CAPACITY, vad_gpu.BAD_PROMISE) == \
        (V.SHORT, V.BAD_RANGE, V.BAD_FRAMES, V.BAD_CAPACITY, V.BAD_PROMISE)
    assert N.SD_VAD_LDS_FRAMES == V.LDS_FRAMES


# ------------------------------------------------------------------ the census of the directory

def test_the_directory_has_two_kernels_with_labelled_launches():
    srcs = {f.name: f.read_text() for f in sorted((CSRC / "vad").glob("*"))}
    assert sorted(srcs) == ["sd_vad.hip", "sd_vad_check.h"]
    text = srcs["sd_vad.hip"]
    kernels = re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", text)
    assert set(kernels) == KERNELS and len(kernels) == 2
    assert re.findall(r'\bSD_CHECK_LAUNCH\("([a-z0-9_]+)"\)', text) == ["vad_energy_kernel", "vad_segments_kernel"]
    assert len(re.findall(r"\bhipLaunchKernelGGL\(", text)) == 2
    code = re.sub(r"//.*", "", text)
    # no atomics at all, no fast arithmetic
    assert "atomic" not in code and "fast-math" not in code and "ffast" not in code and "__fdividef" not in code and "__frcp" not in code
    # the entries refuse through the pure checks and have no argument check of their own
    assert not re.search(r"\bSD_CHECK_ARG\(", code)
    assert len(re.findall(r"\bsd_vad_energy_check\(", code)) == 1 and len(re.findall(r"\bsd_vad_segments_check\(", code)) == 1
    assert len(re.findall(r"\bsd_set_error\(", code)) == 2 and len(re.findall(r"\bsd_vad_workspace_bytes\(", code)) == 1
    # outside the census of csrc/*.hip and of the other directories
    import kernel_census
    assert not KERNELS & {L.kernel_of(lb) for lb in kernel_census.KERNEL_TESTS}
    for other in ("ahc", "cut", "diag", "hdbscan", "tree", "kmeans"):
        theirs = "".join(f.read_text() for f in sorted((CSRC / other).glob("*")))
        assert not KERNELS & set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", theirs))
    for f in CSRC.glob("*.hip"):
        assert not any(k in f.read_text() for k in KERNELS), f.name
    # the check is pure: no HIP, nothing but the status codes
    raw = srcs["sd_vad_check.h"]
    assert re.findall(r'#include [<"]([^>"]+)[>"]', raw) == ["stdio.h", "sd_hip.h"] and "hip" not in re.sub(r"//.*|sd_hip\.h", "", raw).lower()


def test_the_labels_are_asserted_by_the_gpu_tests():
    text = open(os.path.join(HERE, "test_gpu_vad.py")).read()
    assert "pytestmark = pytest.mark.gpu" in text
    assert 'ENERGY_KERNEL = {"vad_energy_kernel"}' in text and 'SEGMENTS_KERNEL = {"vad_segments_kernel"}' in text
    bodies = re.findall(r"^def test_\w+\(.*?(?=^def |^class |^@|\Z)", text, flags=re.M | re.S)
    # every test launches under the log: itself, or through the helpers, which do
    assert len(bodies) >= 8 and all(any(via in b for via in ("expect_launches", "_segments_twice(", "_energy_twice(")) for b in bodies)
    for helper, kernel in (("_segments", "SEGMENTS_KERNEL"), ("_energy", "ENERGY_KERNEL")):
        assert f"expect_launches(exactly={kernel})" in re.search(rf"^def {helper}\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0)
        assert f"{helper}(" in re.search(rf"^def {helper}_twice\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0)


def test_build_list_and_fingerprint_cover_the_directory():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sd_build_native_vad", str(N.PKG_DIR / "build_native.py"))
    bn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bn)
    assert "vad/sd_vad.hip" in bn.SOURCES and all((bn.CSRC / s).exists() for s in bn.SOURCES)
    assert len({os.path.basename(s) for s in bn.SOURCES}) == len(bn.SOURCES)
    assert '(CSRC / "vad").glob("*")' in (N.PKG_DIR / "build_native.py").read_text()


# ------------------------------------------------------------------ the pure check

@pytest.fixture(scope="module")
def pure(tmp_path_factory):
    cxx = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(cxx), "no clang++ on this machine"
    exe = tmp_path_factory.mktemp("vad_check") / "vad_check_pure"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           f"-I{N.PKG_DIR.parent / 'include'}", os.path.join(HERE, "helpers", "vad_check_pure.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(*calls):
        ran = subprocess.run([str(exe), *calls], capture_output=True, text=True)
        assert ran.returncode == 0 and not ran.stderr, (ran.returncode, ran.stderr[-2000:])
        return ran.stdout.splitlines()
    return run


E_NAMES = ("n_groups", "n_frames", "n_signal", "win", "hop", "threshold_db", "slope", "flags")
E_GOOD = (3, 1000, 200000, 480, 160, "-35", "0.6", "-")
S_NAMES = ("n_groups", "n_frames", "seg_cap", "on", "off", "open_len", "close_len", "min_run", "max_gap", "ws_bytes", "flags")
S_GOOD = (3, 1000, 502, "0.6", "0.4", 8, 4, 35, 10, -1, "-")


def _e(**kw):
    return ("energy",) + tuple(kw.get(name, value) for name, value in zip(E_NAMES, E_GOOD))


def _s(**kw):
    return ("segments",) + tuple(kw.get(name, value) for name, value in zip(S_NAMES, S_GOOD))


REFUSALS = [
    (_e(n_groups=0), ARG, "n_groups=0 n_frames=1000 n_signal=200000"),
    (_e(n_frames=-1), ARG, "n_frames=-1"),
    (_e(n_signal=-5), ARG, "n_signal=-5"),
    (_e(win=0), ARG, "win=0 hop=160"),
    (_e(hop=0), ARG, "win=480 hop=0"),
    (_e(threshold_db="nan"), ARG, "threshold_db or slope is not finite"),
    (_e(slope="inf"), ARG, "threshold_db or slope is not finite"),
    (_e(flags="t"), ARG, "null pointer"),
    (_e(flags="f"), ARG, "null pointer"),
    # precedence: the numbers, the frame, the scorer, the pointers
    (_e(n_groups=0, win=0, slope="nan", flags="tf"), ARG, "n_groups=0"),
    (_e(win=0, slope="nan", flags="tf"), ARG, "win=0"),
    (_e(slope="nan", flags="tf"), ARG, "not finite"),
    (_s(n_groups=0), ARG, "n_groups=0 seg_cap=502"),
    (_s(seg_cap=-1), ARG, "seg_cap=-1"),
    (_s(n_frames=-1), ARG, "n_frames=-1"),
    (_s(on="0.4"), ARG, "on=0.4 must exceed off=0.4"),
    (_s(on="0.3"), ARG, "on=0.3 must exceed off=0.4"),
    (_s(on="nan"), ARG, "must exceed"),
    (_s(off="nan"), ARG, "must exceed"),
    (_s(open_len=0), ARG, "open_len=0 close_len=4"),
    (_s(close_len=0), ARG, "open_len=8 close_len=0"),
    (_s(min_run=-1), ARG, "min_run=-1 max_gap=10"),
    (_s(max_gap=-1), ARG, "min_run=35 max_gap=-1"),
    (_s(flags="t"), ARG, "null pointer"),
    (_s(flags="p"), ARG, "null pointer"),
    (_s(flags="s"), ARG, "null pointer"),
    (_s(flags="m"), ARG, "workspace is not 16-byte aligned"),
    (_s(ws_bytes=4015), WS, "workspace of 4015 bytes, seg_cap=502 needs 4016"),
    (_s(ws_bytes=0), WS, "workspace of 0 bytes"),
    # precedence: the groups and the capacity, the frames, the thresholds, the lines, the run rules, the pointers, the alignment, the size
    (_s(n_groups=0, n_frames=-1, on="0", open_len=0, min_run=-1, ws_bytes=0, flags="tpsm"), ARG, "n_groups=0"),
    (_s(n_frames=-1, on="0", open_len=0, min_run=-1, ws_bytes=0, flags="tpsm"), ARG, "n_frames=-1"),
    (_s(on="0", open_len=0, min_run=-1, ws_bytes=0, flags="tpsm"), ARG, "must exceed"),
    (_s(open_len=0, min_run=-1, ws_bytes=0, flags="tpsm"), ARG, "open_len=0"),
    (_s(min_run=-1, ws_bytes=0, flags="tpsm"), ARG, "min_run=-1"),
    (_s(ws_bytes=0, flags="psm"), ARG, "null pointer"),
    (_s(ws_bytes=0, flags="m"), ARG, "workspace is not"),
]
ACCEPTED = [
    (_e(), 0),
    (_e(n_frames=0, flags="f"), 0),                      # no frames: neither the signal nor the probabilities are looked at
    (_e(win=1, hop=1, slope="0", threshold_db="-1e30"), 0),
    (_s(), 8 * 502),
    (_s(n_frames=0, flags="p"), 8 * 502),                # no frames: the probabilities are not looked at
    (_s(seg_cap=0, n_frames=0, flags="psm", ws_bytes=0), 0),   # no capacity: neither the lists nor the workspace are
    (_s(open_len=1, close_len=1, min_run=0, max_gap=0, ws_bytes=10 ** 6), 8 * 502),
    (_s(on="1e-30", off="-1"), 8 * 502),
]


def _call(args):
    return ":".join(str(a) for a in args)


def _entry_name(args):
    return "sd_vad_energy_grouped_f32" if args[0] == "energy" else "sd_vad_segments_grouped"


def test_the_pure_check_refuses_with_code_text_and_precedence(pure):
    out = pure(*[_call(args) for args, _, _ in REFUSALS])
    for (args, code, text), line in zip(REFUSALS, out):
        m = re.fullmatch(r"status=(-?\d+) why=(.*)", line)
        assert m and int(m.group(1)) == code and text in m.group(2) and m.group(2).startswith(_entry_name(args) + ": "), (args, line)
    out = pure(*[_call(args) for args, _ in ACCEPTED])
    for (args, need), line in zip(ACCEPTED, out):
        assert line == f"status=0 need={need}", (args, line)
    assert pure("size:502:3", "size:0:1", "size:-1:1", "size:10:0") == ["4016", "0", "0", "0"]


def test_the_layout_of_the_kernels(pure):
    """A tile of 64 frames stages (count - 1) hop + win floats when they fit into 12 288 (30 ms frames at a 10 ms hop: 10 560), and
    reads in place when they do not; a recording's runs live in LDS up to 16 383 frames"""
    assert pure("layout") == ["256 64 12288 1024 8192 16383"]
    assert pure("stage:64:480:160", "stage:64:400:200", "stage:1:12288:1", "stage:1:12289:1", "stage:64:13001:5", "stage:64:7:3", "stage:0:480:160") == \
        ["10560", "0", "12288", "0", "0", "196", "0"]                     # 63 x 200 + 400 = 13 000 floats do not fit: (400, 200) reads in place
    assert pure("cap:0", "cap:1", "cap:2", "cap:16383", "cap:16384", "cap:-4") == ["0", "1", "1", "8192", "8192", "0"]
    assert (V.LDS_FRAMES + 1) // 2 == 8192


def _energy_entry(lib, n_groups, n_frames, n_signal, win, hop, thr, slope, flags):
    """The same description through the built library: fake non-null pointers, nothing can be launched before the check has passed"""
    t, f = (None if "t" in flags else 0x2000), (None if "f" in flags else 0x1000)
    return lib.sd_vad_energy_grouped_f32(f, n_signal, t, 0x3000, n_groups, win, hop, float(thr), float(slope), 0x4000, n_frames, 0x5000, 0x6000, None)


def _segments_entry(lib, n_groups, n_frames, seg_cap, on, off, open_len, close_len, min_run, max_gap, ws_bytes, flags):
    if ws_bytes < 0:
        ws_bytes = int(lib.sd_vad_segments_workspace_bytes(seg_cap, n_groups))
    return lib.sd_vad_segments_grouped(None if "p" in flags else 0x1000, None if "t" in flags else 0x2000, n_groups, n_frames, float(on), float(off),
                                       open_len, close_len, min_run, max_gap, 0x3000, seg_cap, 0x4000, None if "s" in flags else 0x5000, 0x6000,
                                       0x7000, 0x8000, 0x9004 if "m" in flags else 0x9000, ws_bytes, None)


def test_the_entries_are_wired_to_the_checks():
    """Every refusal comes back from the entry with the same code and text, before anything is launched (a launch on this pointer soup
    would have returned SD_ERR_HIP here and faulted on a GPU); on <= off is among them"""
    lib = N.load()
    for args, code, text in REFUSALS:
        refused((_energy_entry if args[0] == "energy" else _segments_entry)(lib, *args[1:]), code, text)
        assert N.last_error().startswith(_entry_name(args) + ": ")
    names = ("probs", "first_frame", "first_seg", "n_segs", "seg_start", "seg_end", "bad", "ws")
    for name in names:
        p = {k: 0x1000 * (i + 1) for i, k in enumerate(names)}
        p[name] = None
        refused(lib.sd_vad_segments_grouped(p["probs"], p["first_frame"], 3, 1000, 0.6, 0.4, 8, 4, 35, 10, p["first_seg"], 502, p["n_segs"], p["seg_start"],
                                            p["seg_end"], None, p["bad"], p["ws"], 4016, None), ARG, "null pointer")
    names = ("signal", "first_sample", "n_samples", "first_frame", "probs", "bad")
    for name in names:
        p = {k: 0x1000 * (i + 1) for i, k in enumerate(names)}
        p[name] = None
        refused(lib.sd_vad_energy_grouped_f32(p["signal"], 200000, p["first_sample"], p["n_samples"], 3, 480, 160, -35.0, 0.6, p["first_frame"], 1000,
                                              p["probs"], p["bad"], None), ARG, "null pointer")
    with pytest.raises(ValueError, match="on > off"):
        vad_gpu.segments_from_probs_groups(np.zeros(4, np.float32), [0, 4], on=0.4, off=0.4, launch=V.segments_launch)


def test_workspace_formula():
    size = N.load().sd_vad_segments_workspace_bytes
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_vad.h").read()
    assert "sd_vad_segments_workspace_bytes(seg_cap, n_groups) = 8 seg_cap bytes" in header
    for cap, groups in ((0, 1), (1, 1), (502, 3), (1536128, 256), (180000, 1), (2 ** 31 - 1, 5)):
        assert int(size(cap, groups)) == 8 * cap, (cap, groups)
    for cap, groups in ((10, 0), (10, -1), (-1, 3)):
        assert int(size(cap, groups)) == 0, (cap, groups)
    # what the driver asks for: the shares of 256 recordings of two minutes
    counts = vad_gpu.frame_counts([120 * 16000] * 256, 480, 160)
    assert counts[0] == 11998 and int(vad_gpu.run_capacity(counts).sum()) == 256 * 5999


# ------------------------------------------------------------------ the statement of the flags

def test_the_statement_of_the_flags():
    rs = np.random.RandomState(4)
    recs = [rs.uniform(0, 1, n).astype(np.float32) for n in (10, 21, 4)]
    flat = np.concatenate(recs)
    ff, fs = np.array([0, 10, 31, 35]), np.array([0, 5, 16, 18])
    ok = V.segments_entry(flat, ff, fs, 0.6, 0.4, 1, 1, 0, 0)
    assert not ok[4].any() and ok[0].tolist() == [len(V.runs_of(V.hysteresis(p, 0.6, 0.4))) for p in recs]
    small = V.segments_entry(flat, ff, np.array([0, 5, 15, 17]), 0.6, 0.4, 1, 1, 0, 0)
    assert small[4].tolist() == [0, V.BAD_CAPACITY, 0] and small[0][1] == 0 and not small[3][10:31].any()
    for t_ff, t_fs in ((np.array([1, 10, 31, 35]), fs), (np.array([0, 32, 31, 35]), fs), (np.array([0, 10, 31, 34]), fs), (ff, np.array([0, 5, 4, 18])),
                       (ff, np.array([0, 5, 19, 18]))):
        broken = V.segments_entry(flat, t_ff, t_fs, 0.6, 0.4, 1, 1, 0, 0)
        assert broken[4].tolist() == [V.BAD_PROMISE] * 3 and not broken[0].any() and not broken[3].any() and np.all(broken[1] == -1)


# ------------------------------------------------------------------ the routes

def test_the_routes_are_opt_in():
    for fn in (db.diarize_audio, db.diarize_audios, db.Diarizer.__init__):
        assert inspect.signature(fn).parameters["vad"].default == "host"
    text = open(os.path.join(HERE, "..", "tools", "diarize_sharded.py")).read()
    assert '"--vad", default="host", choices=("host", "device")' in text and "vad=a.vad" in text
    assert "vad_gpu.py" in vad.__doc__
    audio = {"waveform": synth.synthetic_conversation(12.0, 2, seed=0).wav, "sample_rate": 16000}
    with pytest.raises(ValueError, match="vad must be 'host' or 'device'"):
        db.diarize_audio(audio, 0.35, 0.1, 2, 6, vad="gpu")
    for call in (lambda: db.diarize_audio(audio, 0.35, 0.1, 2, 6, vad="device", vad_scorer=lambda frames, sr: frames[:, 0]),
                 lambda: db.diarize_audios([audio], 0.35, 0.1, 2, 6, vad="device", vad_scorer=lambda frames, sr: frames[:, 0])):
        with pytest.raises(ValueError, match="segments_from_probs_groups"):
            call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        db.diarize_audio(audio, 0.35, 0.1, 2, 6, vad="device", encoder=lambda w: np.zeros((len(w), 192), np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        db.Diarizer(db.DiarizationParameters(), encoder=lambda w: np.zeros((len(w), 192), np.float32), vad="device")
    assert db.Diarizer(db.DiarizationParameters(), vad="device", clustering="ahc_gpu").vad == "device"
    assert db.Diarizer(db.DiarizationParameters()).vad == "host"
    assert isinstance(vad_gpu.energy_scorer(None), vad.EnergyScorer) and vad_gpu.energy_scorer(vad.EnergyScorer(-30.0, 1.0)).slope == 1.0


def test_there_is_no_cpu_fallback():
    y = synth.synthetic_conversation(12.0, 2, seed=0).wav.astype(np.float32)
    audio = {"waveform": y, "sample_rate": 16000}
    calls = [lambda: vad_gpu.energy_probs_groups(torch.from_numpy(y), [0], [len(y)]),                  # host tensors, GPU or not
             lambda: vad_gpu.segments_from_probs_groups(torch.zeros(10), [0, 10])]
    if not torch.cuda.is_available():
        calls += [lambda: vad_gpu.vad_segments(y), lambda: vad_gpu.vad_segments_groups([y, y]),
                  lambda: db.diarize_audio(audio, 0.35, 0.1, 2, 6, clustering="ahc_gpu", vad="device"),
                  lambda: db.diarize_audios([audio], 0.35, 0.1, 2, 6, vad="device")]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
