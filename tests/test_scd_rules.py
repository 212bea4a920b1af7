"""No-GPU checks of the device speaker-change detection (include/sd_hip_scd.h: sd_scd_split_grouped_f32,
speech-diarization_amd/csrc/scd/, scd_gpu.py, scd="device"): the numpy statement (tests/helpers/scd_ref.py) against pass 2 of
`anti_stick_diarize.scd_split_segments` as it stands and its peak rule against scipy exhaustively, the capacity bound, the header and
its binding table, the census of the new source directory, the pure check (csrc/scd/sd_scd_check.h, built alone with sanitizers) with
its codes and precedence, the workspace formula, the statement of the flags, the seed of the GPU random launch, and the opt-in routes on
stubs."""
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
from scipy.signal import find_peaks

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import hdbscan_grouped_ref as HG  # noqa: E402
import launch_log as L  # noqa: E402
import scd_ref as S  # noqa: E402
from abi_rules import ARG, WS, check_header_and_table, check_versions, refused  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import anti_stick_diarize as asd  # noqa: E402
from speech_diarization_amd import hdbscan_gpu, ops, scd_gpu, speech_encode, synth  # noqa: E402

CSRC = N.PKG_DIR / "csrc"
NAMES = {"sd_scd_abi_version", "sd_scd_split_workspace_bytes", "sd_scd_split_grouped_f32"}
KERNELS = {"scd_split_kernel"}


# ------------------------------------------------------------------ the statement against scipy and against the host

def test_the_peak_rule_equals_find_peaks_exhaustively():
    """Every sequence over {0, 1, 2} of at most 8 values, and each of them with a NaN at each position: exact values, so no margin"""
    checked = 0
    for m in range(1, 9):
        for seq in itertools.product((0.0, 1.0, 2.0), repeat=m):
            for nan_at in range(-1, m):
                x = np.array(seq)
                if nan_at >= 0:
                    x[nan_at] = np.nan
                assert S.peaks_of(x) == find_peaks(x)[0].tolist(), x
                assert S.peaks_of(x.astype(np.float32)) == S.peaks_of(x)
                checked += 1
    assert checked == sum((m + 1) * 3 ** m for m in range(1, 9))
    assert S.peaks_of([0, 1, 1, 0]) == [1] and S.peaks_of([0, 1, 1, 1, 0]) == [2] and S.peaks_of([0, 1, 1]) == [] and S.peaks_of([1, 1, 0]) == []


def _host_pass2(monkeypatch, s32, start, hop_ms, thr, min_speech_ms):
    """Pass 2 of `scd_split_segments` as it stands (its f32 numpy arithmetic, scipy's find_peaks, its greedy loop) on given cosines:
    a signal at 100 Hz, a stub encoder, and `adjacent_cosine` handing out the cosines -> [(start, end)], whether it split"""
    n = len(s32) + 1
    seg = asd.Segment(start, start + 1.0 + 0.2 * (n - 1) + 0.1)         # n windows of 100 samples every 20, ten samples to spare
    y = np.zeros(int(seg.end * 100) + 8, np.float32)

    def cosine(embs, use_gpu):
        assert len(embs) == n and not use_gpu
        return s32
    monkeypatch.setattr(asd, "adjacent_cosine", cosine)
    out = asd.scd_split_segments(y, 100, [seg], win_ms=1000.0, hop_ms=hop_ms, thr=thr, min_speech_ms=min_speech_ms,
                                 encode=lambda w: np.zeros((len(w), 192), np.float32))
    return seg, [(s.start, s.end) for s in out], not (len(out) == 1 and out[0] is seg)


def test_the_statement_equals_pass_2_of_the_host(monkeypatch):
    """20 000 random cases (four families of cosines, 3-59 windows, thr in {1.0, 1.25, 1.5, 2.0}, hop 200 ms, min_speech 1 s): the
    pieces are equal, value for value, for every case whose value margin is at least 1e-4 (every case whose margin is, and those
    whose only close decisions are about times: scd_ref.py); at most 1 % of the cases may lie below it.
    With seed 0: 20 000 cases, 32 left out (0.16 %), 0 disagreements among the rest, 14 860 cases split."""
    rs = np.random.RandomState(0)
    cases = left_out = split = 0
    for _ in range(20000):
        n = rs.randint(3, 60)
        s32 = S.cosine_family(S.FAMILIES[rs.randint(4)], n - 1, rs)
        thr, start = S.THRS[rs.randint(4)], 0.25 * rs.randint(0, 40)
        seg, host, did = _host_pass2(monkeypatch, s32, start, 200.0, thr, 1000.0)
        kept, pieces, margin, value_margin = S.split_from_cosines(s32, seg.start, seg.end, 200.0, thr, 1.0)
        cases += 1
        assert margin <= value_margin
        if value_margin < S.MARGIN:
            left_out += 1
            continue
        assert host == pieces and did == bool(kept), (s32.tolist(), thr, start, margin)
        split += did
    print(f"{cases} cases, {left_out} left out ({100.0 * left_out / cases:.3f} %), {split} split")
    assert S.MARGIN == 1e-4 and left_out <= 0.01 * cases and split > 10000


def test_the_capacity_bound_is_reached_by_an_alternating_sequence():
    """max(1, n // 2) pieces: an alternating sequence of distances has a peak at every odd index, (m - 1) // 2 of them, and with
    min_speech_s = 0 every cut and the tail emit a piece"""
    for n in range(0, 41):
        s = np.array([1.0 if i % 2 == 0 else 0.0 for i in range(max(n - 1, 0))], np.float32)
        kept, pieces = S.split_from_cosines(s, 10.0, 30.0, 200.0, -1e9, 0.0)[:2]
        assert len(kept) == max(n - 2, 0) // 2 and len(pieces) == S.capacity(n) == int(scd_gpu.piece_capacity(n)), n
    for m in range(1, 9):                                                  # and no sequence has more peaks
        for seq in itertools.product((0.0, 1.0, 2.0), repeat=m):
            assert len(S.peaks_of(seq)) <= (m - 1) // 2


# ------------------------------------------------------------------ ABI

def test_header_and_binding_table_name_the_same_exported_entries():
    others = (N.PROTOTYPES, N.SPECTRAL_PROTOTYPES, N.AHC_PROTOTYPES, N.HDBSCAN_PROTOTYPES, N.DIAG_PROTOTYPES, N.TRACE_PROTOTYPES, N.TREE_ENTRIES,
              N.CUT_ENTRIES, N.KMEANS_ENTRIES, N.VAD_ENTRIES)
    assert check_header_and_table("sd_hip_scd.h", N.SCD_ENTRIES, others) == NAMES
    assert ops._SCD_LAUNCHABLE == NAMES and not NAMES & (ops._LAUNCHABLE | ops._CUT_LAUNCHABLE | ops._KMEANS_LAUNCHABLE | ops._VAD_LAUNCHABLE)
    assert '("sd_hip_scd.h", SCD_ENTRIES, "sd_scd_abi_version", SD_SCD_ABI_VERSION, "SCD ")' in open(N.__file__).read()
    with pytest.raises(ValueError, match="not an entry"):
        ops.launch("sd_scd_split", torch.zeros(1))


def test_the_new_version_is_one_and_every_other_is_untouched():
    assert N.SD_SCD_ABI_VERSION == 1
    check_versions(sd_scd_abi_version=1, sd_vad_abi_version=1, sd_kmeans_abi_version=1, sd_cut_abi_version=1, sd_tree_abi_version=1,
                   sd_abi_version=11, sd_spectral_abi_version=1, sd_ahc_abi_version=1, sd_hdbscan_abi_version=1, sd_diag_abi_version=1,
                   sd_trace_abi_version=3)
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_scd.h").read()
    assert re.search(r"#define\s+SD_SCD_ABI_VERSION\s+1\b", header)
    for name, value in (("BAD_CAPACITY", S.BAD_CAPACITY), ("BAD_PROMISE", S.BAD_PROMISE), ("LDS_ROWS", S.LDS_ROWS)):
        assert re.search(rf"#define\s+SD_SCD_{name}\s+{value}\b", header), name
    assert (scd_gpu.BAD_CAPACITY, scd_gpu.BAD_PROMISE) == (S.BAD_CAPACITY, S.BAD_PROMISE) and N.SD_SCD_LDS_ROWS == S.LDS_ROWS


# ------------------------------------------------------------------ the census of the directory

def test_the_directory_has_one_kernel_with_a_labelled_launch():
    srcs = {f.name: f.read_text() for f in sorted((CSRC / "scd").glob("*"))}
    assert sorted(srcs) == ["sd_scd.hip", "sd_scd_check.h"]
    text = srcs["sd_scd.hip"]
    kernels = re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", text)
    assert kernels == ["scd_split_kernel"]
    assert re.findall(r'\bSD_CHECK_LAUNCH\("([a-z0-9_]+)"\)', text) == ["scd_split_kernel"]
    assert len(re.findall(r"\bhipLaunchKernelGGL\(", text)) == 1
    code = re.sub(r"//.*", "", text)
    # no atomics at all, no fast arithmetic, and contraction off for the whole file
    assert "atomic" not in code and "fast-math" not in code and "ffast" not in code and "__fdividef" not in code and "__frcp" not in code
    assert code.count("#pragma clang fp contract(off)") == 1 and code.index("#pragma clang fp contract(off)") < code.index("namespace {")
    # the cosine is the device code of sd_adjacent_cosine_f32, stated once
    assert len(re.findall(r"\bsd_wave_pair_cosine\(", code)) == 1
    pool = re.sub(r"//.*", "", (CSRC / "sd_pool.hip").read_text())
    body = re.search(r"void adjacent_cosine_kernel\(.*?\n}\n", pool, flags=re.S).group(0)
    assert "sd_wave_pair_cosine(" in body and "sqrtf" not in body
    assert len(re.findall(r"float sd_wave_pair_cosine\(", (CSRC / "sd_common.h").read_text())) == 1
    # the entry refuses through the pure check and has no argument check of its own
    assert not re.search(r"\bSD_CHECK_ARG\(", code)
    assert len(re.findall(r"\bsd_scd_check\(", code)) == 1 and len(re.findall(r"\bsd_set_error\(", code)) == 1
    assert len(re.findall(r"\bsd_scd_workspace_bytes\(", code)) == 1
    # outside the census of csrc/*.hip and of the other directories
    import kernel_census
    assert not KERNELS & {L.kernel_of(lb) for lb in kernel_census.KERNEL_TESTS}
    for other in ("ahc", "cut", "diag", "hdbscan", "tree", "kmeans", "vad"):
        theirs = "".join(f.read_text() for f in sorted((CSRC / other).glob("*")))
        assert not KERNELS & set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", theirs))
    for f in CSRC.glob("*.hip"):
        assert not any(k in f.read_text() for k in KERNELS), f.name
    # the check is pure: no HIP, nothing but the status codes
    raw = srcs["sd_scd_check.h"]
    assert re.findall(r'#include [<"]([^>"]+)[>"]', raw) == ["stdio.h", "sd_hip.h"] and "hip" not in re.sub(r"//.*|sd_hip\.h", "", raw).lower()


def test_the_label_is_asserted_by_the_gpu_tests():
    text = open(os.path.join(HERE, "test_gpu_scd.py")).read()
    assert "pytestmark = pytest.mark.gpu" in text and 'KERNEL = {"scd_split_kernel"}' in text
    bodies = re.findall(r"^def test_\w+\(.*?(?=^def |^class |^@|\Z)", text, flags=re.M | re.S)
    # every test launches under the log: itself, or through the helpers, which do
    assert len(bodies) >= 10 and all(any(via in b for via in ("expect_launches", "_check(", "_split_twice(")) for b in bodies)
    assert "expect_launches(exactly=KERNEL)" in re.search(r"^def _split\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0)
    assert "_split(" in re.search(r"^def _split_twice\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0)
    assert "_split_twice(" in re.search(r"^def _check\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0)


def test_build_list_and_fingerprint_cover_the_directory():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sd_build_native_scd", str(N.PKG_DIR / "build_native.py"))
    bn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bn)
    assert "scd/sd_scd.hip" in bn.SOURCES and all((bn.CSRC / s).exists() for s in bn.SOURCES)
    assert len({os.path.basename(s) for s in bn.SOURCES}) == len(bn.SOURCES)
    assert '(CSRC / "scd").glob("*")' in (N.PKG_DIR / "build_native.py").read_text()


# ------------------------------------------------------------------ the pure check

@pytest.fixture(scope="module")
def pure(tmp_path_factory):
    cxx = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(cxx), "no clang++ on this machine"
    exe = tmp_path_factory.mktemp("scd_check") / "scd_check_pure"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           f"-I{N.PKG_DIR.parent / 'include'}", os.path.join(HERE, "helpers", "scd_check_pure.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(*calls):
        ran = subprocess.run([str(exe), *calls], capture_output=True, text=True)
        assert ran.returncode == 0 and not ran.stderr, (ran.returncode, ran.stderr[-2000:])
        return ran.stdout.splitlines()
    return run


C_NAMES = ("ld", "dim", "n_rows", "n_segs", "piece_cap", "hop_ms", "thr", "min_speech_s", "eps", "ws_bytes", "flags")
C_GOOD = (192, 192, 1000, 40, 520, "200", "1.25", "1", "1e-8", -1, "-")
ENTRY = "sd_scd_split_grouped_f32"


def _c(**kw):
    return ("split",) + tuple(kw.get(name, value) for name, value in zip(C_NAMES, C_GOOD))


REFUSALS = [
    (_c(n_segs=0), ARG, "n_segs=0 n_rows=1000"),
    (_c(n_segs=-3), ARG, "n_segs=-3"),
    (_c(n_rows=-1), ARG, "n_rows=-1"),
    (_c(piece_cap=-1), ARG, "piece_cap=-1"),
    (_c(dim=0), ARG, "dim=0 ld=192"),
    (_c(ld=191), ARG, "dim=192 ld=191"),
    (_c(hop_ms="nan"), ARG, "hop_ms, min_speech_s or eps is not finite"),
    (_c(hop_ms="inf"), ARG, "is not finite"),
    (_c(min_speech_s="-inf"), ARG, "is not finite"),
    (_c(min_speech_s="nan"), ARG, "is not finite"),
    (_c(eps="inf"), ARG, "is not finite"),
    (_c(eps="nan"), ARG, "is not finite"),
    (_c(thr="nan"), ARG, "thr is not a number"),
    (_c(flags="t"), ARG, "null pointer"),
    (_c(flags="r"), ARG, "null pointer"),
    (_c(flags="p"), ARG, "null pointer"),
    (_c(flags="m"), ARG, "workspace is not 16-byte aligned"),
    (_c(ws_bytes=15999), WS, "workspace of 15999 bytes, n_rows=1000 needs 16000"),
    (_c(ws_bytes=0), WS, "workspace of 0 bytes"),
    # precedence: the segments and the rows, the capacity, the row shape, the parameters, thr, the pointers, the alignment, the size
    (_c(n_segs=0, piece_cap=-1, dim=0, hop_ms="nan", thr="nan", ws_bytes=0, flags="trpm"), ARG, "n_segs=0"),
    (_c(piece_cap=-1, dim=0, hop_ms="nan", thr="nan", ws_bytes=0, flags="trpm"), ARG, "piece_cap=-1"),
    (_c(dim=0, hop_ms="nan", thr="nan", ws_bytes=0, flags="trpm"), ARG, "dim=0"),
    (_c(hop_ms="nan", thr="nan", ws_bytes=0, flags="trpm"), ARG, "is not finite"),
    (_c(thr="nan", ws_bytes=0, flags="trpm"), ARG, "thr is not a number"),
    (_c(ws_bytes=0, flags="rpm"), ARG, "null pointer"),
    (_c(ws_bytes=0, flags="m"), ARG, "workspace is not"),
]
ACCEPTED = [
    (_c(), 16000),
    (_c(thr="inf"), 16000),                              # an infinite threshold switches the stage off, as the callers' 1e9 does
    (_c(thr="-inf", min_speech_s="-5", hop_ms="-200", eps="0"), 16000),
    (_c(n_rows=0, flags="rm", ws_bytes=0), 0),           # no rows: neither the rows nor the workspace are looked at
    (_c(piece_cap=0, flags="p"), 16000),                 # no capacity: the piece lists are not looked at (every segment is flagged)
    (_c(dim=5, ld=8, ws_bytes=10 ** 6), 16000),
    (_c(dim=1, ld=1), 16000),
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
    assert pure("size:1000:40", "size:0:1", "size:-1:1", "size:10:0") == ["16000", "0", "0", "0"]


def test_the_layout_of_the_kernel(pure):
    """256 threads; the distances, cuts and chain of a segment live in LDS up to 2 048 rows (at most 1 023 cuts); the workspace holds
    the cuts, then the distances, then the chain; a segment of n rows needs max(1, n // 2) pieces"""
    assert pure("layout") == ["256 2048 1024"]
    assert pure("offsets:1000", "offsets:0", "offsets:3") == ["8000 12000", "0 0", "24 36"]
    ns = (-4, 0, 1, 2, 3, 4, 5, 2048, 2049)
    assert pure(*[f"cap:{n}" for n in ns]) == [str(S.capacity(n)) for n in ns] == ["1", "1", "1", "1", "1", "2", "2", "1024", "1024"]
    assert (S.LDS_ROWS - 2) // 2 < 1024


def _entry(lib, ld, dim, n_rows, n_segs, piece_cap, hop_ms, thr, min_speech_s, eps, ws_bytes, flags):
    """The same description through the built library: fake non-null pointers, nothing can be launched before the check has passed"""
    if ws_bytes < 0:
        ws_bytes = int(lib.sd_scd_split_workspace_bytes(n_rows, n_segs))
    t, r, p = (None if "t" in flags else 0x2000), (None if "r" in flags else 0x1000), (None if "p" in flags else 0x7000)
    return lib.sd_scd_split_grouped_f32(r, ld, dim, n_rows, t, n_segs, 0x3000, 0x4000, float(hop_ms), float(thr), float(min_speech_s), float(eps),
                                        0x5000, piece_cap, 0x6000, 0x6100, p, 0x8000, None, None, 0x9000, 0xa004 if "m" in flags else 0xa000,
                                        ws_bytes, None)


def test_the_entry_is_wired_to_the_check():
    """Every refusal comes back from the entry with the same code and text, before anything is launched (a launch on this pointer soup
    would have returned SD_ERR_HIP here and faulted on a GPU)"""
    lib = N.load()
    for args, code, text in REFUSALS:
        refused(_entry(lib, *args[1:]), code, text)
        assert N.last_error().startswith(ENTRY + ": ")
    names = ("rows", "first_row", "seg_start", "seg_end", "first_piece", "n_peaks", "n_pieces", "piece_start", "piece_end", "bad", "ws")
    for name in names:
        p = {k: 0x1000 * (i + 1) for i, k in enumerate(names)}
        p[name] = None
        refused(lib.sd_scd_split_grouped_f32(p["rows"], 192, 192, 1000, p["first_row"], 40, p["seg_start"], p["seg_end"], 200.0, 1.25, 1.0, 1e-8,
                                             p["first_piece"], 520, p["n_peaks"], p["n_pieces"], p["piece_start"], p["piece_end"], None, None,
                                             p["bad"], p["ws"], 16000, None), ARG, "null pointer")
    for kw in (dict(hop_ms=0.0), dict(hop_ms=-200.0)):
        with pytest.raises(ValueError, match="hop_ms must be positive"):
            scd_gpu.split_rows_groups(np.zeros((4, 8), np.float32), [0, 4], [0.0], [1.0], thr=1.0, min_speech_ms=1000.0, launch=S.numpy_launch, **kw)


def test_workspace_formula():
    size = N.load().sd_scd_split_workspace_bytes
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_scd.h").read()
    assert "sd_scd_split_workspace_bytes(n_rows, n_segs) = 16 n_rows bytes" in header
    for rows, segs in ((0, 1), (1, 1), (1000, 40), (384000, 15360), (18000, 1), (2 ** 31 - 1, 5)):
        assert int(size(rows, segs)) == 16 * rows, (rows, segs)
    for rows, segs in ((10, 0), (10, -1), (-1, 3)):
        assert int(size(rows, segs)) == 0, (rows, segs)


# ------------------------------------------------------------------ the statement of the flags, the driver

def test_the_statement_of_the_flags_and_the_driver():
    rs = np.random.RandomState(4)
    counts = [0, 1, 2, 3, 12, 30, 7]
    fr = np.concatenate([[0], np.cumsum(counts)])
    fp = np.concatenate([[0], np.cumsum([S.capacity(n) for n in counts])])
    rows = np.concatenate([S.rows_with_cosines(S.cosine_family("drops", n - 1, rs), 8, rs) for n in counts if n])
    starts = np.arange(len(counts)) * 100.0
    ends = starts + 1.0 + 0.2 * np.maximum(np.array(counts) - 1, 0)
    cos = S.sims_layout([S.cosines64(rows[a:b]).astype(np.float32) if b > a else None for a, b in zip(fr[:-1], fr[1:])])
    assert len(cos) == len(rows)
    ok = S.split_entry(cos, fr, starts, ends, 200.0, 1.0, 0.5, fp)
    assert not ok["bad"].any() and ok["n_peaks"][:4].tolist() == [0, 0, 0, 0] and ok["n_pieces"][:4].tolist() == [1, 1, 1, 1] and ok["n_peaks"][4:6].all()
    assert ok["mask"].sum() == ok["n_peaks"].sum() and np.isnan(ok["piece_start"]).sum() == fp[-1] - ok["n_pieces"].sum()
    small = fp.copy()
    small[5] -= 1                                        # segment 4 has one slot fewer than 12 // 2; segment 5 gets it
    flagged = S.split_entry(cos, fr, starts, ends, 200.0, 1.0, 0.5, small)
    assert flagged["bad"].tolist() == [0, 0, 0, 0, S.BAD_CAPACITY, 0, 0] and flagged["n_pieces"][4] == 0 and not flagged["mask"][fr[4]:fr[5]].any()
    assert not S.promise_holds([0, 5, 4, 9], 9, [0, 1, 2, 3], 3) and not S.promise_holds([0, 4, 9], 9, [1, 2, 3], 3) and S.promise_holds(fr, len(rows), fp, fp[-1])
    # the driver on the numpy launch: the same pieces, the tables it builds, and its refusals
    seen = []

    def launch(rows_, first_row, seg_start, seg_end, first_piece, hop_ms, thr, min_speech_s):
        seen.append((first_row.tolist(), first_piece.tolist(), hop_ms, thr, min_speech_s))
        return S.numpy_launch(rows_, first_row, seg_start, seg_end, first_piece, hop_ms, thr, min_speech_s)
    got = scd_gpu.split_rows_groups(rows, fr, starts, ends, 200.0, 1.0, 500.0, launch=launch)
    assert seen == [(fr.tolist(), fp.tolist(), 200.0, 1.0, 0.5)] and len(got) == len(counts)
    for g, (k, pieces) in enumerate(got):
        q = fp[g]
        assert k == ok["n_peaks"][g] and pieces == list(zip(ok["piece_start"][q:q + len(pieces)], ok["piece_end"][q:q + len(pieces)]))
        assert len(pieces) == ok["n_pieces"][g] and (k or pieces == [(starts[g], ends[g])])
    with pytest.raises(ValueError, match="first_row must run from 0"):
        scd_gpu.split_rows_groups(rows, fr[:-1], starts[:-1], ends[:-1], 200.0, 1.0, 500.0, launch=launch)
    with pytest.raises(ValueError, match="one time per segment"):
        scd_gpu.split_rows_groups(rows, fr, starts[:-1], ends, 200.0, 1.0, 500.0, launch=launch)
    with pytest.raises(RuntimeError, match=r"refused segment\(s\) \[1\]: flags \[1\]"):
        scd_gpu.split_rows_groups(rows, fr, starts, ends, 200.0, 1.0, 500.0,
                                  launch=lambda *a: (np.zeros(7, np.int32), np.zeros(7, np.int32), np.zeros(21), np.zeros(21), np.eye(7, dtype=np.int32)[1]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scd_gpu.split_rows_groups(torch.from_numpy(rows), fr, starts, ends, 200.0, 1.0, 500.0)      # host rows, GPU or not


def test_the_seed_of_the_gpu_random_launch_keeps_the_reference_within_the_cap():
    """The random launches of tests/test_gpu_scd.py, their cosines stated in float64: at most 1 % of their segments lie below the
    margin, and most of them split"""
    below = split = total = 0
    for make in (S.random_launch, S.long_segment):
        rows, fr, starts, ends = make()
        counts = np.diff(fr)
        if make is S.random_launch:
            assert len(counts) == 200 and counts.min() >= 3 and counts.max() <= 40 and rows[0].shape[1] == 16
        else:
            assert counts.tolist() == [S.LDS_ROWS + 1] and rows[0].shape[1] == 8
        cos = S.sims_layout([S.cosines64(r).astype(np.float32) for r in rows])
        for thr in S.THRS:
            out = S.split_entry(cos, fr, starts, ends, 200.0, thr, 1.0, np.concatenate([[0], np.cumsum([S.capacity(n) for n in counts])]))
            below += int((out["value_margin"] < S.MARGIN).sum())
            split += int((out["n_peaks"] > 0).sum())
            total += len(counts)
    print(f"{total} segments, {below} below the margin, {split} split")
    assert below <= 0.01 * total and split > 400, (below, split)
    text = open(os.path.join(HERE, "test_gpu_scd.py")).read()
    assert "S.random_launch()" in text and "S.long_segment()" in text


# ------------------------------------------------------------------ the routes, on stubs

def _fft_rows(w):
    return np.stack([np.abs(np.fft.rfft(r, 382))[:192] for r in np.asarray(w, dtype=np.float32)]).astype(np.float32)


class _StubEncoder:
    """`HipEcapaEncoder.encode_windows` on the host: the windows read in place, embedded by an FFT"""
    def __init__(self):
        self.calls = []

    def encode_windows(self, signal, starts, n, rows_per_call=8192, to_host=True):
        assert to_host is False
        self.calls.append(len(starts))
        return torch.from_numpy(_fft_rows(np.stack([signal[a:a + n] for a in starts])))


def _vad(y, sr, **kw):
    if not np.any(y):
        return []
    total = len(y) / sr
    return [(0.0, total)] if total < 2.0 else [(0.3, total / 2), (total / 2 + 0.2, total - 0.1)]


@pytest.fixture()
def stubs(monkeypatch):
    enc, splits = _StubEncoder(), []

    def launch(rows, *a):
        splits.append(int(rows.shape[0]))
        return S.numpy_launch(rows.numpy(), *a)
    monkeypatch.setattr(speech_encode, "using_ecapa_encoder", lambda: enc)
    monkeypatch.setattr(speech_encode, "ecapa_encode_batches", lambda batches: [_fft_rows(b) for b in batches])
    monkeypatch.setattr(scd_gpu, "split_launch", launch)
    product_factory = hdbscan_gpu.HdbscanGpuClusterer.factory
    monkeypatch.setattr(hdbscan_gpu.HdbscanGpuClusterer, "factory", staticmethod(lambda operator=None: product_factory(operator=HG.NumpyGroupedRows())))
    return enc, splits


def _times(segs):
    return [(s.start, s.end) for s in segs]


def test_scd_device_routes_on_stubs(stubs):
    """`scd_split_segments(scd="device")` against the host route on the same stub embeddings (margins of the statement: at least
    1e-4 is asserted), `scd_split_segments_many` with one split call for the folder, unsplit segments returned as the same objects"""
    enc, splits = stubs
    ys = [synth.synthetic_conversation(20.0, 2, seed=0).wav.astype(np.float32), np.zeros(3 * 16000, np.float32),
          synth.synthetic_conversation(12.0, 3, seed=1).wav.astype(np.float32), synth.synthetic_conversation(20.0, 2, seed=0).wav[:int(0.9 * 16000)].astype(np.float32)]
    lists = [[asd.Segment(s, e) for s, e in _vad(y, 16000)] or [asd.Segment(0.0, 1.3)] for y in ys]   # silence: two windows
    for thr in (1.0, 1.5):
        alone = []
        for y, segs in zip(ys, lists):
            splits.clear()
            dev = asd.scd_split_segments(y, 16000, segs, thr=thr, scd="device")
            host = asd.scd_split_segments(y, 16000, segs, thr=thr, encode=_fft_rows)
            assert len(splits) <= 1
            # the margins of this recording's segments under the statement, from the same float64 cosines
            for seg in segs:
                a = int(seg.start * 16000)
                n = max(0, 1 + (len(y[a:int(seg.end * 16000)]) - 16000) // 3200)
                if n >= 3:
                    rows = _fft_rows(np.stack([y[a + 3200 * i: a + 3200 * i + 16000] for i in range(n)]))
                    assert S.split_from_cosines(S.cosines64(rows).astype(np.float32), seg.start, seg.end, 200.0, thr, 1.0)[3] >= S.MARGIN
            assert _times(dev) == _times(host)
            assert all((d is s) == (h is s) for s in segs for d, h in zip(dev, host) if d.start == s.start and d.end == s.end)
            alone.append(dev)
        splits.clear(), enc.calls.clear()
        many = asd.scd_split_segments_many(ys, 16000, lists, thr=thr)
        assert len(splits) == 1 and len(enc.calls) == 2 and splits[0] == sum(enc.calls)       # ONE split for the folder; windows per recording
        assert [_times(m) for m in many] == [_times(a) for a in alone]
        assert many[1][0] is lists[1][0] and many[3][0] is lists[3][0]                         # nothing to split: the same objects
        assert [_times(m) for m in asd.scd_split_segments_many(ys, 16000, lists, thr=thr, encode=_fft_rows, scd="host")] == [_times(a) for a in alone]
    assert sum(len(a) for a in alone) >= sum(len(s) for s in lists)
    splits.clear()
    assert asd.scd_split_segments_many([], 16000, []) == [] and asd.scd_split_segments(ys[0], 16000, [], scd="device") == [] and not splits


def test_diarize_many_with_the_device_scd_equals_diarize_per_recording(stubs):
    enc, splits = stubs
    ys = [synth.synthetic_conversation(20.0, 2, seed=0).wav, np.zeros(3 * 16000, np.float32), synth.synthetic_conversation(12.0, 3, seed=1).wav,
          synth.synthetic_conversation(20.0, 2, seed=0).wav[:int(0.9 * 16000)]]
    kw = dict(vad_segments=_vad, scd_thr=1.0, reseg=0, scd="device")
    want = [asd.diarize(y, clusterer="hdbscan_gpu", **kw) for y in ys]
    assert len(splits) == 2                                                # the two conversations; the others have no segment of 3 windows
    splits.clear(), enc.calls.clear()
    got = asd.diarize_many(ys, **kw)
    assert len(splits) == 1 and len(enc.calls) == 2                        # ONE split call for the folder
    assert [[(s.start, s.end, s.spk) for s in g] for g in got] == [[(s.start, s.end, s.spk) for s in w] for w in want]
    assert got[1] == [] and len(got[3]) == 1 and len(got[0]) > 2
    assert asd.diarize_many([], **kw) == []


def test_the_routes_are_opt_in_and_the_signatures_agree():
    p_one, p_many = inspect.signature(asd.diarize).parameters, inspect.signature(asd.diarize_many).parameters
    assert list(p_many)[1:] == list(p_one)[1:] and list(p_one)[-1] == "scd"
    for p in (p_one, p_many, inspect.signature(asd.scd_split_segments).parameters):
        assert p["scd"].default == "host" and p["scd"].kind == inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(asd.scd_split_segments_many).parameters["scd"].default == "device"
    y = synth.synthetic_conversation(12.0, 2, seed=0).wav.astype(np.float32)
    segs = [asd.Segment(0.0, 12.0)]
    for call in (lambda: asd.scd_split_segments(y, 16000, segs, encode=_fft_rows, scd="device"),
                 lambda: asd.scd_split_segments_many([y], 16000, [segs], encode=_fft_rows),
                 lambda: asd.diarize(y, encode=_fft_rows, vad_segments=_vad, scd="device"),
                 lambda: asd.diarize_many([y], encode=_fft_rows, vad_segments=_vad, scd="device")):
        with pytest.raises(ValueError, match="scd='device' splits the window embeddings of the HIP encoder"):
            call()
    for call in (lambda: asd.scd_split_segments(y, 16000, segs, encode=_fft_rows, scd="gpu"), lambda: asd.diarize(y, encode=_fft_rows, scd="gpu"),
                 lambda: asd.diarize_many([y], encode=_fft_rows, scd="gpu")):
        with pytest.raises(ValueError, match="scd must be 'host' or 'device'"):
            call()
    # the default route is untouched: the same objects and values with and without the keyword
    a = asd.scd_split_segments(y, 16000, segs, thr=1.0, encode=_fft_rows)
    b = asd.scd_split_segments(y, 16000, segs, thr=1.0, encode=_fft_rows, scd="host")
    assert _times(a) == _times(b) and len(a) > 1
    assert "scd_gpu" in asd.scd_split_segments.__doc__ and "ONE split" in asd.diarize_many.__doc__


def test_there_is_no_cpu_fallback():
    y = synth.synthetic_conversation(12.0, 2, seed=0).wav.astype(np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scd_gpu.split_rows_groups(torch.zeros(10, 8), [0, 10], [0.0], [3.0], 200.0, 1.0, 1000.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scd_split_grouped(torch.zeros(10, 8), torch.zeros(2, dtype=torch.int32), torch.zeros(1, dtype=torch.float64),
                              torch.zeros(1, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), 5, 200.0, 1.0, 1.0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            asd.scd_split_segments(y, 16000, [asd.Segment(0.0, 12.0)], scd="device")
