"""No-GPU checks of the device speaker turns (include/sd_hip_turns.h: sd_turns_grouped, speech-diarization_amd/csrc/turns/,
turns_gpu.py, turns="device"): the numpy statement (tests/helpers/turns_ref.py) against `cluster.relabel_by_first_appearance` plus
`diarization_baseline.labels_to_turns` as they stand, on recordings built with `speech_windows` itself and on hand-made ones, with no
case excluded; the driver's packing through the statement; the header and its binding table; the census of the new source directory;
the pure check (csrc/turns/sd_turns_check.h, built alone with sanitizers) with its codes and precedence; the refusals of the loaded
library; the workspace formula; and the opt-in keyword."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import launch_log as L  # noqa: E402
import turns_ref as T  # noqa: E402
from abi_rules import ARG, WS, check_header_and_table, check_versions, refused  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import cluster, ops, turns_gpu  # noqa: E402
from speech_diarization_amd import diarization_baseline as db  # noqa: E402

CSRC = N.PKG_DIR / "csrc"
NAMES = {"sd_turns_abi_version", "sd_turns_workspace_bytes", "sd_turns_grouped"}
KERNELS = {"turns_kernel"}
LABELS = {"turns_kernel/lds", "turns_kernel/ws"}
ENTRY = "sd_turns_grouped"


# ------------------------------------------------------------------ the statement against the host

def _host(speech, centres, regions, labels, frame_s=0.01):
    new = cluster.relabel_by_first_appearance(labels)
    return new, db.labels_to_turns(speech, centres, regions, new, frame_s)


def _statement(speech, centres, regions, labels, frame_s=0.01, times=turns_gpu.turn_times):
    """The statement on one recording, fed as the driver feeds the entry -> (new labels, turns, the integer runs)"""
    nr = len(speech)
    rfw = np.append(np.searchsorted(regions, np.arange(nr)), len(centres))
    start = np.array([s for s, _ in speech], np.float64)
    frames = np.array([max(1, int(round((e - s) / frame_s))) for s, e in speech], np.int64)
    assert T.promise_of_a_recording(rfw, np.asarray(centres, np.float64), start, frames, frame_s)
    new = T.relabel(labels)
    runs = T.runs_of_a_recording(rfw, np.asarray(centres, np.float64), start, frames, frame_s, new)
    return new, times(speech, *runs, frame_s), runs


def _random_speech(rs, sr, win_s):
    """Speech regions of every kind `speech_windows` tells apart: shorter than the window (one centred window), between the window and
    the window plus both margins (no margin taken), longer (the margin taken; a covering tail window unless the length fits the hop),
    and of a single frame; starts on the millisecond grid or off it"""
    speech, t = [], float(rs.uniform(0.0, 0.5))
    for _ in range(rs.randint(1, 7)):
        kind = rs.randint(5)
        length = (rs.uniform(0.2, win_s), rs.uniform(win_s, win_s + 0.3), rs.uniform(win_s + 0.3, 9.0), rs.uniform(0.004, 0.016),
                  win_s + 0.3 + 0.25 * rs.randint(0, 12))[kind]
        s = round(t, 3) if rs.randint(2) else t
        speech.append((s, s + length))
        t = s + length + rs.uniform(0.05, 1.0)
    return speech, int((t + 0.5) * sr)


def test_the_statement_equals_the_host_on_recordings_from_speech_windows():
    """2 400 random recordings through `speech_windows` (window 2 s, hop 0.25 s; every third with window 1 s, hop 0.1 s): the relabelled
    labels are equal and the turns are equal as tuples, the vectorised times equal the scalar expression, and none is left out.  The
    kinds of region are counted, so that each is known to have been met."""
    rs = np.random.RandomState(0)
    seen = {"tail": 0, "short": 0, "margin": 0, "no_margin": 0, "one_frame": 0, "on_grid": 0, "off_grid": 0, "minus_one": 0, "runs": 0}
    sr = 16000
    for case in range(2400):
        win_s, hop_s = (1.0, 0.1) if case % 3 == 2 else (2.0, 0.25)
        speech, n_samples = _random_speech(rs, sr, win_s)
        starts, centres, regions = db.speech_windows(speech, n_samples, sr, win_s, hop_s)
        k = rs.randint(1, 5)
        labels = np.repeat(rs.randint(-1, k, len(starts)), rs.randint(1, 5))[:len(starts)] if case % 2 else rs.randint(-1, k, len(starts))
        labels = np.minimum(labels, len(starts) - 1)
        assert len(labels) == len(starts)
        want_labels, want = _host(speech, centres, regions, labels)
        new, got, runs = _statement(speech, centres, regions, labels)
        assert np.array_equal(new, want_labels), case
        assert got == want, (case, speech)
        assert _statement(speech, centres, regions, labels, times=turns_gpu.turn_times_scalar)[1] == want
        assert len(got) <= len(starts)
        win, hop, margin = int(win_s * sr), int(hop_s * sr), int(round(0.15 * sr))
        for r, (s, e) in enumerate(speech):
            a, b = int(round(s * sr)), min(int(round(e * sr)), n_samples)
            seen["short"] += b - a < win
            seen["no_margin"] += win <= b - a < win + 2 * margin
            seen["margin"] += b - a >= win + 2 * margin
            if b - a >= win + 2 * margin:
                seen["tail"] += (b - a - 2 * margin - win) % hop != 0
            seen["one_frame"] += max(1, int(round((e - s) / 0.01))) == 1
            seen["on_grid" if s == round(s, 3) else "off_grid"] += 1
        seen["minus_one"] += bool((labels < 0).any())
        seen["runs"] += len(got)
    print(seen)
    assert all(v >= 100 for v in seen.values()), seen


def _hand_made():
    """(speech, centres, regions, labels, frame_s, owners without a frame): windows that own no frame at the start, in the middle and
    at the end of a region (two centres one sample apart), and exact ties, where the first of two equidistant centres wins"""
    one = 1.0 / 16000
    cases = []
    # middle: three centres one sample apart between two frames; the middle one lies between no two frame times
    cases.append(([(1.0, 3.0)], [1.5, 2.0021, 2.0021 + one, 2.0021 + 2 * one, 2.5], [0] * 5, [0, 1, 2, 3, 4], 0.01, {2}))
    # start: the first window lies before a centre that is already nearer to frame 0
    cases.append(([(1.0, 3.0)], [0.5, 0.5 + one, 2.0], [0] * 3, [0, 1, 0], 0.01, {0}))
    # end: the last window lies one sample after its predecessor, past the last frame
    cases.append(([(1.0, 3.0)], [2.0, 3.5, 3.5 + one], [0] * 3, [0, 1, 2], 0.01, {2}))
    # all three in two regions of one recording, with a region of one window between them and labels with -1
    cases.append(([(0.0, 2.0), (2.5, 2.6), (3.0, 5.0)], [-1.0, -1.0 + one, 1.0, 1.0 + one, 1.0 + 2 * one, 2.55, 4.0, 6.0, 6.0 + one],
                  [0, 0, 0, 0, 0, 1, 2, 2, 2], [3, 3, -1, 2, 3, -1, 0, 3, 1], 0.01, {0, 1, 3, 7, 8}))
    # exact ties: frame_s = 0.25 and centres 0.75 apart put frames exactly between two centres; the first centre wins
    cases.append(([(0.0, 2.0)], [0.0, 0.75, 1.5], [0] * 3, [0, 1, 2], 0.25, set()))
    cases.append(([(4.0, 6.0), (8.0, 9.0)], [4.125, 4.625, 5.125, 8.0, 8.25, 8.5, 8.75], [0, 0, 0, 1, 1, 1, 1], [1, 1, 0, 0, 1, 0, 1], 0.25, set()))
    cases.append(([(0.0, 1.0)], [0.125, 0.375, 0.375 + 2.0 ** -30, 0.625], [0] * 4, [0, 1, 2, 3], 0.25, {2}))
    return [(sp, np.array(c), np.array(r), np.array(lab), fs, own) for sp, c, r, lab, fs, own in cases]


def test_the_statement_equals_the_host_on_hand_made_windows():
    for speech, centres, regions, labels, frame_s, without in _hand_made():
        want_labels, want = _host(speech, centres, regions, labels, frame_s)
        new, got, runs = _statement(speech, centres, regions, labels, frame_s)
        assert np.array_equal(new, want_labels) and got == want, (speech, got, want)
        assert _statement(speech, centres, regions, labels, frame_s, times=turns_gpu.turn_times_scalar)[1] == want
        # the windows said to own no frame: the brute-force owners never name them, and every other window is named
        owners = set()
        for r, (s, e) in enumerate(speech):
            sel = np.flatnonzero(regions == r)
            t = s + (np.arange(max(1, int(round((e - s) / frame_s)))) + 0.5) * frame_s
            owners |= set(sel[np.argmin(np.abs(t[:, None] - centres[sel][None, :]), axis=1)].tolist())
        assert set(range(len(centres))) - owners == without, (speech, owners)
    # the tie itself: frame 1 of the first tie case lies at 0.375, exactly between 0.0 and 0.75, and goes to window 0
    speech, centres, regions, labels, frame_s, _ = _hand_made()[4]
    assert abs(0.375 - centres[0]) == abs(0.375 - centres[1])
    assert _statement(speech, centres, regions, labels, frame_s)[2][1].tolist() == [0, 2, 5]


def test_relabel_is_the_hosts():
    rs = np.random.RandomState(1)
    for _ in range(300):
        labels = rs.randint(-2, rs.randint(1, 9), rs.randint(0, 40))
        assert np.array_equal(T.relabel(labels), cluster.relabel_by_first_appearance(labels))
    assert T.relabel([5, -3, 5, 0, 2, 0]).tolist() == [0, -1, 0, 1, 2, 1]


def test_the_capacity_is_reached_by_alternating_labels_and_the_margin_is_stated():
    rec = T.even_recording([7, 0, 1, 12], np.arange(20) % 2)
    rfw, centre, start, frames, labels = rec
    runs = T.runs_of_a_recording(rfw, centre, start, frames, 0.01, T.relabel(labels))
    assert len(runs[0]) == 20 and runs[0].tolist() == [0] * 7 + [2] + [3] * 12
    assert T.promise_of_a_recording(rfw, centre, start, frames, 0.01)
    # the promises: equal centres, a decreasing slice, a frame count of 0, a non-finite start or centre, a gap below E * 2^-40
    c = centre.copy()
    c[3] = c[2]
    assert not T.promise_of_a_recording(rfw, c, start, frames, 0.01)
    assert not T.promise_of_a_recording([0, 8, 7, 8, 20], centre, start, frames, 0.01)
    assert not T.promise_of_a_recording(rfw, centre, start, [25, 25, 0, 25], 0.01)
    for bad in (np.nan, np.inf):
        s = start.copy()
        s[0] = bad
        assert not T.promise_of_a_recording(rfw, centre, s, frames, 0.01)
        c = centre.copy()
        c[-1] = bad
        assert not T.promise_of_a_recording(rfw, c, start, frames, 0.01)
    c = centre.copy()
    c[1] = c[0] + 2.0 ** -44
    assert c[1] > c[0] and not T.promise_of_a_recording(rfw, c, start, frames, 0.01)
    assert T.MARGIN == 2.0 ** -40 and "E * 2^-40" in open(N.PKG_DIR.parent / "include" / "sd_hip_turns.h").read()


# ------------------------------------------------------------------ the driver, through the statement

def _folder():
    """speech, centres, regions, labels per recording: two from `speech_windows`, an empty recording (no speech), a recording with
    speech and no windows, and one whose middle region has no windows"""
    rs = np.random.RandomState(2)
    out = []
    for n_regions in (3, 5):
        speech, n_samples = _random_speech(rs, 16000, 2.0)
        _, centres, regions = db.speech_windows(speech, n_samples, 16000, 2.0, 0.25)
        out.append((speech, centres, regions, rs.randint(-1, 3, len(centres))))
    out.insert(1, ([], None, None, np.zeros(0, int)))
    out.append(([(0.5, 1.5), (2.0, 2.4)], np.zeros(0), np.zeros(0, np.int64), np.zeros(0, int)))
    out.append(([(0.0, 2.0), (3.0, 4.0), (5.0, 8.0)], np.array([0.5, 1.0, 1.5, 6.0, 6.5, 7.0]), np.array([0, 0, 0, 2, 2, 2]), np.array([2, 2, 0, 0, -1, 2])))
    return out


def test_the_driver_packs_and_unpacks_through_the_statement():
    folder = _folder()
    seen = []

    def launch(*tables):
        seen.append([np.asarray(t).copy() if not isinstance(t, float) else t for t in tables])
        return T.numpy_launch(*tables)
    got = turns_gpu.labels_to_turns_groups(*[list(x) for x in zip(*folder)], launch=launch)
    assert len(seen) == 1 and len(got) == len(folder)
    fw, fr, rfw, centre, start, frames, frame_s, labels = seen[0]
    sizes = [0 if c is None else len(c) for _, c, _, _ in folder]
    assert fw.tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist() and fr.tolist() == np.concatenate([[0], np.cumsum([len(s) for s, _, _, _ in folder])]).tolist()
    assert len(rfw) == fr[-1] + 1 and rfw[-1] == fw[-1] == len(centre) == len(labels) and len(start) == len(frames) == fr[-1] and frame_s == 0.01
    assert rfw[fr[4]:fr[5] + 1].tolist() == [fw[4], fw[4] + 3, fw[4] + 3, fw[5]]                     # the region without windows
    assert T.tables_hold(fw, fr, len(centre), len(start))
    for (speech, centres, regions, lab), (new, turns) in zip(folder, got):
        want_labels, want = _host(speech, np.zeros(0) if centres is None else centres, np.zeros(0, int) if regions is None else regions, lab)
        assert np.array_equal(new, want_labels) and new.dtype == want_labels.dtype and turns == want
    assert got[1][1] == [] and got[3][1] == [] and len(got[4][1]) == 5
    assert turns_gpu.labels_to_turns_groups([], [], [], [], launch=launch) == [] and len(seen) == 1


def test_the_driver_refuses_what_the_entry_does_not_promise():
    speech = [(0.0, 2.0), (3.0, 5.0)]
    c, lab = np.array([0.5, 1.0, 3.5, 4.0]), np.zeros(4, int)
    with pytest.raises(ValueError, match="must not decrease"):
        turns_gpu.labels_to_turns_groups([speech], [c], [np.array([0, 1, 0, 1])], [lab], launch=T.numpy_launch)
    with pytest.raises(ValueError, match=r"must lie in \[0, 2\)"):
        turns_gpu.labels_to_turns_groups([speech], [c], [np.array([0, 0, 1, 2])], [lab], launch=T.numpy_launch)
    for centres in (np.array([0.5, 0.5, 3.5, 4.0]), np.array([0.5, 1.0, 4.0, 3.5])):
        with pytest.raises(ValueError, match="increase strictly inside a region"):
            turns_gpu.labels_to_turns_groups([speech], [centres], [np.array([0, 0, 1, 1])], [lab], launch=T.numpy_launch)
    assert turns_gpu.labels_to_turns_groups([speech], [np.array([1.0, 1.5, 0.5, 0.75])], [np.array([0, 0, 1, 1])], [lab], launch=T.numpy_launch)
    with pytest.raises(ValueError, match="per recording"):
        turns_gpu.labels_to_turns_groups([speech], [c, c], [np.zeros(4, int)], [lab], launch=T.numpy_launch)
    with pytest.raises(ValueError, match="frame_s must be positive"):
        turns_gpu.labels_to_turns_groups([speech], [c], [np.array([0, 0, 1, 1])], [lab], frame_s=0.0, launch=T.numpy_launch)
    with pytest.raises(RuntimeError, match=r"refused recording\(s\) \[0\]: flags \[1\]"):       # a label that is no window's index
        turns_gpu.labels_to_turns_groups([speech], [c], [np.array([0, 0, 1, 1])], [np.array([0, 4, 0, 0])], launch=T.numpy_launch)
    if not torch.cuda.is_available():                    # there is no implicit CPU route
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            turns_gpu.labels_to_turns_groups([speech], [c], [np.array([0, 0, 1, 1])], [lab])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.turns_grouped(*(torch.zeros(2, dtype=torch.int32) for _ in range(3)), torch.zeros(0, dtype=torch.float64),
                          torch.zeros(1, dtype=torch.float64), torch.ones(1, dtype=torch.int32), 0.01, torch.zeros(0, dtype=torch.int32))


def test_the_statement_of_the_flags():
    recs = [T.even_recording([3, 2], [0, 1, 1, 0, 2]), T.even_recording([], []), T.even_recording([4], [1, 1, -1, 0])]
    tables = T.tables_of(recs)
    ok = T.turns_entry(*tables[:6], 0.01, tables[6])
    assert not ok["bad"].any() and ok["n_runs"].tolist() == [4, 0, 3] and ok["new_labels"].tolist() == [0, 1, 1, 0, 2, 0, 0, -1, 1]
    assert ok["run_region"].tolist() == [0, 0, 1, 1, -7, 0, 0, 0, -7] and ok["run_first"][:4].tolist() == [0, 25, 0, 25] and ok["run_end"][:4].tolist() == [25, 75, 25, 50]
    labels = tables[6].copy()
    labels[6] = 4                                        # recording 2 has 4 windows
    flagged = T.turns_entry(*tables[:6], 0.01, labels)
    assert flagged["bad"].tolist() == [0, 0, T.BAD_LABEL] and flagged["n_runs"].tolist() == [4, 0, 0] and (flagged["new_labels"][5:] == -7).all()
    fw = tables[0].copy()
    fw[1] = 6
    assert T.turns_entry(fw, *tables[1:6], 0.01, tables[6])["bad"].tolist() == [T.BAD_PROMISE] * 3
    centre = tables[3].copy()
    centre[1] = centre[0]
    both = T.turns_entry(*tables[:3], centre, *tables[4:6], 0.01, labels)
    assert both["bad"].tolist() == [T.BAD_PROMISE, 0, T.BAD_LABEL]
    assert (turns_gpu.BAD_LABEL, turns_gpu.BAD_PROMISE) == (T.BAD_LABEL, T.BAD_PROMISE)


# ------------------------------------------------------------------ ABI

def test_header_and_binding_table_name_the_same_exported_entries():
    others = (N.PROTOTYPES, N.SPECTRAL_PROTOTYPES, N.AHC_PROTOTYPES, N.HDBSCAN_PROTOTYPES, N.DIAG_PROTOTYPES, N.TRACE_PROTOTYPES, N.TREE_ENTRIES,
              N.CUT_ENTRIES, N.KMEANS_ENTRIES, N.VAD_ENTRIES, N.SCD_ENTRIES)
    assert check_header_and_table("sd_hip_turns.h", N.TURNS_ENTRIES, others) == NAMES
    assert ops._TURNS_LAUNCHABLE == NAMES
    assert not NAMES & (ops._LAUNCHABLE | ops._CUT_LAUNCHABLE | ops._KMEANS_LAUNCHABLE | ops._VAD_LAUNCHABLE | ops._SCD_LAUNCHABLE)
    assert '("sd_hip_turns.h", TURNS_ENTRIES, "sd_turns_abi_version", SD_TURNS_ABI_VERSION, "turns ")' in open(N.__file__).read()
    with pytest.raises(ValueError, match="not an entry"):
        ops.launch("sd_turns", torch.zeros(1))


def test_the_new_version_is_one_and_every_other_is_untouched():
    assert N.SD_TURNS_ABI_VERSION == 1
    check_versions(sd_turns_abi_version=1, sd_scd_abi_version=1, sd_vad_abi_version=1, sd_kmeans_abi_version=1, sd_cut_abi_version=1,
                   sd_tree_abi_version=1, sd_abi_version=11, sd_spectral_abi_version=1, sd_ahc_abi_version=1, sd_hdbscan_abi_version=1,
                   sd_diag_abi_version=1, sd_trace_abi_version=3)
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_turns.h").read()
    assert re.search(r"#define\s+SD_TURNS_ABI_VERSION\s+1\b", header)
    for name, value in (("BAD_LABEL", T.BAD_LABEL), ("BAD_PROMISE", T.BAD_PROMISE), ("LDS_WINDOWS", T.LDS_WINDOWS)):
        assert re.search(rf"#define\s+SD_TURNS_{name}\s+{value}\b", header), name
    assert N.SD_TURNS_LDS_WINDOWS == T.LDS_WINDOWS


# ------------------------------------------------------------------ the census of the directory

def test_the_directory_has_one_kernel_with_a_labelled_launch():
    srcs = {f.name: f.read_text() for f in sorted((CSRC / "turns").glob("*"))}
    assert sorted(srcs) == ["sd_turns.hip", "sd_turns_check.h"]
    text = srcs["sd_turns.hip"]
    assert re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", text) == ["turns_kernel"]
    launch = re.findall(r"\bSD_CHECK_LAUNCH\((.*)\);", text)
    assert len(launch) == 1 and set(re.findall(r'"([a-z_/]+)"', launch[0])) == LABELS
    assert len(re.findall(r"\bhipLaunchKernelGGL\(", text)) == 1
    code = re.sub(r"//.*", "", text)
    # integer atomics on the flags and the table only; no fast arithmetic; contraction off for the whole file
    assert set(re.findall(r"\b(atomic[A-Za-z]*)\(", code)) == {"atomicOr", "atomicMin"} and not re.search(r"\bfloat\b", code)
    assert "fast-math" not in code and "ffast" not in code and "__fdividef" not in code and "__frcp" not in code
    assert code.count("#pragma clang fp contract(off)") == 1 and code.index("#pragma clang fp contract(off)") < code.index("namespace {")
    # the entry refuses through the pure check and has no argument check of its own
    assert not re.search(r"\bSD_CHECK_ARG\(", code)
    assert len(re.findall(r"\bsd_turns_check\(", code)) == 1 and len(re.findall(r"\bsd_set_error\(", code)) == 1
    assert len(re.findall(r"\bsd_turns_ws_bytes\(", code)) == 1
    # outside the census of csrc/*.hip and of the other directories
    import kernel_census
    assert not KERNELS & {L.kernel_of(lb) for lb in kernel_census.KERNEL_TESTS}
    for other in ("ahc", "cut", "diag", "hdbscan", "tree", "kmeans", "vad", "scd"):
        theirs = "".join(f.read_text() for f in sorted((CSRC / other).glob("*")))
        assert not KERNELS & set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", theirs))
    for f in CSRC.glob("*.hip"):
        assert not any(k in f.read_text() for k in KERNELS), f.name
    # the check is pure: no HIP, nothing but the status codes
    raw = srcs["sd_turns_check.h"]
    assert re.findall(r'#include [<"]([^>"]+)[>"]', raw) == ["stdio.h", "sd_hip.h"] and "hip" not in re.sub(r"//.*|sd_hip\.h", "", raw).lower()


def test_the_labels_are_asserted_by_the_gpu_tests():
    text = open(os.path.join(HERE, "test_gpu_turns.py")).read()
    assert "pytestmark = pytest.mark.gpu" in text and 'LDS, WS = {"turns_kernel/lds"}, {"turns_kernel/ws"}' in text
    bodies = re.findall(r"^def test_\w+\(.*?(?=^def |^class |^@|\Z)", text, flags=re.M | re.S)
    # every test launches under the log: itself, or through the helpers, which do
    assert len(bodies) >= 10 and all(any(via in b for via in ("expect_launches", "_check(", "_run_twice(", "_run(")) for b in bodies)
    assert "expect_launches(exactly=label)" in re.search(r"^def _run\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0)
    assert "_run(" in re.search(r"^def _run_twice\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0)
    assert "_run_twice(" in re.search(r"^def _check\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0)


def test_build_list_and_fingerprint_cover_the_directory():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sd_build_native_turns", str(N.PKG_DIR / "build_native.py"))
    bn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bn)
    assert "turns/sd_turns.hip" in bn.SOURCES and all((bn.CSRC / s).exists() for s in bn.SOURCES)
    assert len({os.path.basename(s) for s in bn.SOURCES}) == len(bn.SOURCES)
    assert '(CSRC / "turns").glob("*")' in (N.PKG_DIR / "build_native.py").read_text()


# ------------------------------------------------------------------ the pure check

@pytest.fixture(scope="module")
def pure(tmp_path_factory):
    cxx = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(cxx), "no clang++ on this machine"
    exe = tmp_path_factory.mktemp("turns_check") / "turns_check_pure"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           f"-I{N.PKG_DIR.parent / 'include'}", os.path.join(HERE, "helpers", "turns_check_pure.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(*calls):
        ran = subprocess.run([str(exe), *calls], capture_output=True, text=True)
        assert ran.returncode == 0 and not ran.stderr, (ran.returncode, ran.stderr[-2000:])
        return ran.stdout.splitlines()
    return run


C_NAMES = ("n_recordings", "n_regions", "n_windows", "frame_s", "ws_bytes", "flags")
C_GOOD = (40, 900, 10000, "0.01", -1, "-")


def _c(**kw):
    return ("turns",) + tuple(kw.get(name, value) for name, value in zip(C_NAMES, C_GOOD))


REFUSALS = [
    (_c(n_recordings=0), ARG, "n_recordings=0 n_windows=10000"),
    (_c(n_recordings=-3), ARG, "n_recordings=-3"),
    (_c(n_windows=-1), ARG, "n_windows=-1"),
    (_c(n_regions=-1), ARG, "n_regions=-1"),
    (_c(frame_s="0"), ARG, "frame_s is not a positive finite number"),
    (_c(frame_s="-0.01"), ARG, "frame_s is not"),
    (_c(frame_s="nan"), ARG, "frame_s is not"),
    (_c(frame_s="inf"), ARG, "frame_s is not"),
    (_c(flags="t"), ARG, "null pointer"),
    (_c(flags="r"), ARG, "null pointer"),
    (_c(flags="w"), ARG, "null pointer"),
    (_c(flags="n"), ARG, "null pointer"),
    (_c(flags="m"), ARG, "workspace is not 16-byte aligned"),
    (_c(ws_bytes=79999), WS, "workspace of 79999 bytes, n_windows=10000 needs 80000"),
    (_c(ws_bytes=0), WS, "workspace of 0 bytes"),
    (_c(n_windows=4097, ws_bytes=32775), WS, "n_windows=4097 needs 32776"),
    # precedence: the recordings and the windows, the regions, the frame length, the pointers, the alignment, the size
    (_c(n_recordings=0, n_regions=-1, frame_s="nan", ws_bytes=0, flags="trwnm"), ARG, "n_recordings=0"),
    (_c(n_regions=-1, frame_s="nan", ws_bytes=0, flags="trwnm"), ARG, "n_regions=-1"),
    (_c(frame_s="nan", ws_bytes=0, flags="trwnm"), ARG, "frame_s is not"),
    (_c(ws_bytes=0, flags="wnm"), ARG, "null pointer"),
    (_c(ws_bytes=0, flags="nm"), ARG, "null pointer"),
    (_c(ws_bytes=0, flags="m"), ARG, "workspace is not"),
]
ACCEPTED = [
    (_c(), 80000),
    (_c(ws_bytes=10 ** 6), 80000),
    (_c(n_windows=4097), 32776),                         # one window above the LDS tables: the first launch that needs a workspace
    (_c(n_windows=4096, ws_bytes=0, flags="nm"), 0),     # at it: none, and `ws` is not looked at
    (_c(n_windows=4095, ws_bytes=0, flags="n"), 0),
    (_c(n_windows=0, ws_bytes=0, flags="wnm"), 0),       # no windows: the window arrays are not looked at
    (_c(n_regions=0, n_windows=0, ws_bytes=0, flags="rwn"), 0),
    (_c(n_recordings=1, n_regions=1, n_windows=1, frame_s="1e-300", ws_bytes=0), 0),
]


def _call(args):
    return ":".join(str(a) for a in args)


def test_the_pure_check_refuses_with_code_text_and_precedence(pure):
    out = pure(*[_call(args) for args, _, _ in REFUSALS])
    for (args, code, text), line in zip(REFUSALS, out):
        m = re.fullmatch(r"status=(-?\d+) why=(.*)", line)
        assert m and int(m.group(1)) == code and text in m.group(2) and m.group(2).startswith(ENTRY + ": "), (args, line)
    out = pure(*[_call(args) for args, _ in ACCEPTED])
    for (args, need), line in zip(ACCEPTED, out):
        assert line == f"status=0 need={need}", (args, line)
    assert pure("size:10000:40", "size:4096:1", "size:4097:1", "size:0:1", "size:-1:1", "size:10000:0") == ["80000", "0", "32776", "0", "0", "0"]
    assert pure("layout") == [f"256 {T.LDS_WINDOWS}"] and pure("offset:10000", "offset:0") == ["40000", "0"]


def _entry(lib, n_recordings, n_regions, n_windows, frame_s, ws_bytes, flags):
    """The same description through the built library: fake non-null pointers, nothing can be launched before the check has passed"""
    if ws_bytes < 0:
        ws_bytes = int(lib.sd_turns_workspace_bytes(n_windows, n_recordings))
    t, r, w = (None if "t" in flags else 0x1000), (None if "r" in flags else 0x4000), (None if "w" in flags else 0x6000)
    ws = None if "n" in flags else (0xf004 if "m" in flags else 0xf000)
    return lib.sd_turns_grouped(t, 0x2000, n_recordings, 0x3000, n_regions, w, n_windows, r, 0x5000, float(frame_s), 0x7000, 0x8000, 0x9000,
                                0xa000, 0xb000, 0xc000, 0xd000, 0xe000, ws, ws_bytes, None)


def test_the_entry_is_wired_to_the_check():
    """Every refusal comes back from the entry with the same code and text, before anything is launched (a launch on this pointer soup
    would have returned SD_ERR_HIP here and faulted on a GPU)"""
    lib = N.load()
    for args, code, text in REFUSALS:
        refused(_entry(lib, *args[1:]), code, text)
        assert N.last_error().startswith(ENTRY + ": ")
    names = ("first_window", "first_region", "region_first_window", "centre", "region_start", "n_frames", "labels", "new_labels", "n_runs",
             "run_region", "run_first", "run_end", "run_label", "bad", "ws")
    for name in names:
        p = {k: 0x1000 * (i + 1) for i, k in enumerate(names)}
        p[name] = None
        refused(lib.sd_turns_grouped(p["first_window"], p["first_region"], 40, p["region_first_window"], 900, p["centre"], 10000, p["region_start"],
                                     p["n_frames"], 0.01, p["labels"], p["new_labels"], p["n_runs"], p["run_region"], p["run_first"], p["run_end"],
                                     p["run_label"], p["bad"], p["ws"], 80000, None), ARG, "null pointer")


def test_workspace_formula():
    size = N.load().sd_turns_workspace_bytes
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_turns.h").read()
    assert "sd_turns_workspace_bytes(n_windows, n_recordings) = 8 n_windows bytes when n_windows > SD_TURNS_LDS_WINDOWS" in header
    for windows, recs in ((0, 1), (1, 1), (4096, 3), (4097, 1), (128000, 256), (2 ** 31 - 1, 5)):
        assert int(size(windows, recs)) == (8 * windows if windows > T.LDS_WINDOWS else 0), (windows, recs)
    for windows, recs in ((10, 0), (10, -1), (-1, 3)):
        assert int(size(windows, recs)) == 0, (windows, recs)


# ------------------------------------------------------------------ the keyword

def test_the_route_is_opt_in_and_keyword_only():
    for fn in (db.diarize_audio, db.diarize_audios, db.Diarizer.__init__):
        p = inspect.signature(fn).parameters["turns"]
        assert p.default == "host" and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    for call in (lambda: db.diarize_audio({"waveform": np.zeros(16000, np.float32), "sample_rate": 16000}, 0.35, 0.1, 2, 6, turns="gpu"),
                 lambda: db.diarize_audios([], 0.35, 0.1, 2, 6, turns="gpu"), lambda: db.Diarizer(db.DiarizationParameters(), turns="gpu")):
        with pytest.raises(ValueError, match="turns must be 'host' or 'device'"):
            call()
    encoder = lambda w: np.zeros((len(w), 192), np.float32)      # noqa: E731
    with pytest.raises(RuntimeError, match="turns='device' runs on the HIP path"):
        db.Diarizer(db.DiarizationParameters(), encoder=encoder, turns="device")
    with pytest.raises(RuntimeError, match="turns='device' runs on the HIP path"):
        db.diarize_audio({"waveform": np.zeros(16000, np.float32), "sample_rate": 16000}, 0.35, 0.1, 2, 6, encoder=encoder, turns="device")
    assert db.Diarizer(db.DiarizationParameters(), turns="device").turns == "device" and db.Diarizer(db.DiarizationParameters()).turns == "host"
    assert "--turns" in open(N.PKG_DIR.parent / "tools" / "diarize_sharded.py").read()
    assert "turns_gpu" in db.diarize_audio.__doc__ and "ONE" in db.diarize_audios.__doc__
