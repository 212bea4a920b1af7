"""No-GPU checks of the bounded cut of the AHC device route (include/sd_hip_cut.h: sd_ahc_cut_grouped, speech-diarization_amd/csrc/cut/,
`ahc_gpu.ahc_cosine_rows / ahc_cosine_groups(..., min_clusters=, max_clusters=)`, `speaker_bounds=` of the public calls): the header
and its binding table, the untouched versions and tables, the census of the new source directory, the pure check (csrc/cut/
sd_cut_check.h, built alone with sanitizers) with its codes and precedence, the workspace formula, the numpy statement of the entry
against scipy, and the bounded drivers run on the CPU through a numpy operator that has `cut`."""
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
import ahc_cut_ref as CR  # noqa: E402
import ahc_grouped_ref as AG  # noqa: E402
import ahc_ref as A  # noqa: E402
import launch_log as L  # noqa: E402
from abi_rules import ARG, WS, check_header_and_table, check_versions, refused  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import ahc_gpu, ops  # noqa: E402
from speech_diarization_amd import diarization_baseline as db  # noqa: E402

CSRC = N.PKG_DIR / "csrc"
CUT = CSRC / "cut"
NAMES = {"sd_cut_abi_version", "sd_ahc_cut_workspace_bytes", "sd_ahc_cut_grouped"}
ENTRY = "sd_ahc_cut_grouped"
KERNEL = "ahc_cut_grouped_kernel"


# ------------------------------------------------------------------ ABI

def test_header_and_binding_table_name_the_same_exported_entries():
    others = (N.PROTOTYPES, N.SPECTRAL_PROTOTYPES, N.AHC_PROTOTYPES, N.HDBSCAN_PROTOTYPES, N.DIAG_PROTOTYPES, N.TRACE_PROTOTYPES, N.TREE_ENTRIES)
    assert check_header_and_table("sd_hip_cut.h", N.CUT_ENTRIES, others) == NAMES
    # `ops.launch` takes them from a set of their own; the six *_PROTOTYPES tables, their union and the tree table's set stay what they were
    assert ops._LAUNCHABLE == ops._ENTRIES | set(N.TREE_ENTRIES) and not NAMES & ops._LAUNCHABLE and ops._CUT_LAUNCHABLE == NAMES
    assert sorted(k for k in vars(N) if k.endswith("PROTOTYPES")) == ["AHC_PROTOTYPES", "DIAG_PROTOTYPES", "HDBSCAN_PROTOTYPES", "PROTOTYPES",
                                                                     "SPECTRAL_PROTOTYPES", "TRACE_PROTOTYPES"]
    assert '("sd_hip_cut.h", CUT_ENTRIES, "sd_cut_abi_version", SD_CUT_ABI_VERSION, "cut ")' in open(N.__file__).read()
    with pytest.raises(ValueError, match="not an entry"):
        ops.launch("sd_ahc_cut", torch.zeros(1))


def test_the_new_version_is_one_and_every_other_is_untouched():
    assert N.SD_CUT_ABI_VERSION == 1
    check_versions(sd_cut_abi_version=1, sd_tree_abi_version=1, sd_abi_version=11, sd_spectral_abi_version=1, sd_ahc_abi_version=1,
                   sd_hdbscan_abi_version=1, sd_diag_abi_version=1, sd_trace_abi_version=3)
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_cut.h").read()
    assert re.search(r"#define\s+SD_CUT_ABI_VERSION\s+1\b", header)
    assert set(N.AHC_PROTOTYPES) == {"sd_ahc_abi_version", "sd_ahc_nearest_workspace_bytes", "sd_ahc_nearest_f32", "sd_ahc_merge_f32",
                                     "sd_ahc_nearest_grouped_workspace_bytes", "sd_ahc_nearest_grouped_f32"}


# ------------------------------------------------------------------ the census of the directory

def test_the_directory_has_one_kernel_with_one_labelled_launch():
    srcs = {f.name: f.read_text() for f in sorted(CUT.glob("*"))}
    assert sorted(srcs) == ["sd_ahc_cut.hip", "sd_cut_check.h"]
    text = srcs["sd_ahc_cut.hip"]
    kernels = set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", text))
    assert kernels == {KERNEL}
    assert re.findall(r'\bSD_CHECK_LAUNCH\("([a-z0-9_]+)"\)', text) == [KERNEL]
    assert len(re.findall(r"\bhipLaunchKernelGGL\(", text)) == 1
    code = re.sub(r"//.*", "", text)
    # integer atomics on LDS only: every atomic is an atomicAdd on a __shared__ histogram or counter
    atomics = re.findall(r"\batomic\w*\(&(\w+)", code)
    assert atomics and set(atomics) <= {"s_hist", "s_count"} and len(atomics) == len(re.findall(r"atomic", code)), atomics
    for name in set(atomics):
        assert re.search(rf"__shared__ int [^;]*\b{name}\b", code), name
    assert "fast-math" not in code and not re.search(r"atomic\w*\([^)]*float", code)
    # the entry refuses through the one pure check and has no argument check of its own
    assert not re.search(r"\bSD_CHECK_ARG\(", code) and len(re.findall(r"\bsd_cut_check\(", code)) == 1
    assert len(re.findall(r"\bsd_set_error\(", code)) == 1 and len(re.findall(r"\bsd_cut_workspace_bytes\(", code)) == 1
    # outside the census of csrc/*.hip and of the other directories
    import kernel_census
    assert not kernels & {L.kernel_of(lb) for lb in kernel_census.KERNEL_TESTS}
    for other in ("ahc", "diag", "hdbscan", "tree"):
        theirs = "".join(f.read_text() for f in sorted((CSRC / other).glob("*")))
        assert not kernels & set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", theirs))
    for f in CSRC.glob("*.hip"):
        assert KERNEL not in f.read_text(), f.name
    # the check is pure: no HIP, nothing but the status codes
    raw = srcs["sd_cut_check.h"]
    assert re.findall(r'#include [<"]([^>"]+)[>"]', raw) == ["stdio.h", "sd_hip.h"] and "hip" not in re.sub(r"//.*|sd_hip\.h", "", raw).lower()


def test_the_label_is_asserted_by_the_gpu_tests():
    text = open(os.path.join(HERE, "test_gpu_ahc_cut.py")).read()
    assert "pytestmark = pytest.mark.gpu" in text
    assert re.search(rf'KERNEL = "{KERNEL}"', text)
    bodies = re.findall(r"^def test_\w+\(.*?(?=^def |^class |\Z)", text, flags=re.M | re.S)
    # every test launches under the log: itself, or through _run (and _check over it) or _drive, which do
    assert len(bodies) >= 6 and all(any(via in b for via in ("expect_launches", "_run(", "_check(", "_drive(")) for b in bodies)
    for helper in ("_run", "_drive"):
        assert "expect_launches(exactly={KERNEL})" in re.search(rf"^def {helper}\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0), helper
    assert "_run(" in re.search(r"^def _check\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0)
    assert "expect_launches(exactly={KERNEL})" in text


def test_build_list_and_fingerprint_cover_the_directory():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sd_build_native_cut", str(N.PKG_DIR / "build_native.py"))
    bn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bn)
    assert "cut/sd_ahc_cut.hip" in bn.SOURCES and all((bn.CSRC / s).exists() for s in bn.SOURCES)
    assert len({os.path.basename(s) for s in bn.SOURCES}) == len(bn.SOURCES)
    assert '(CSRC / "cut").glob("*")' in (N.PKG_DIR / "build_native.py").read_text()


# ------------------------------------------------------------------ the pure check

@pytest.fixture(scope="module")
def pure(tmp_path_factory):
    cxx = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(cxx), "no clang++ on this machine"
    exe = tmp_path_factory.mktemp("cut_check") / "cut_check_pure"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           f"-I{N.PKG_DIR.parent / 'include'}", os.path.join(HERE, "helpers", "cut_check_pure.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(*calls):
        ran = subprocess.run([str(exe), *calls], capture_output=True, text=True)
        assert ran.returncode == 0 and not ran.stderr, (ran.returncode, ran.stderr[-2000:])
        return ran.stdout.splitlines()
    return run


# (n_groups, n_merges, n_rows, cos_thr, ws_bytes (-1: the need), flags) -> (status, text in the message)
REFUSALS = [
    ((0, 5, 10, "0.5", -1, "-"), ARG, "n_groups=0 n_merges=5 n_rows=10"),
    ((-2, 5, 10, "0.5", -1, "-"), ARG, "n_groups=-2"),
    ((3, 5, -1, "0.5", -1, "-"), ARG, "n_rows=-1"),
    ((3, -5, 10, "0.5", -1, "-"), ARG, "n_merges=-5"),
    ((3, 11, 10, "0.5", -1, "-"), ARG, "n_merges=11 exceeds n_rows=10"),
    ((3, 5, 10, "nan", -1, "-"), ARG, "cos_thr is not a number"),
    ((3, 5, 10, "0.5", -1, "t"), ARG, "null pointer"),
    ((3, 5, 10, "0.5", -1, "e"), ARG, "null pointer"),
    ((3, 5, 10, "0.5", -1, "r"), ARG, "null pointer"),
    ((3, 5, 10, "0.5", -1, "w"), ARG, "null pointer"),
    ((3, 5, 10, "0.5", -1, "m"), ARG, "workspace is not 16-byte aligned"),
    ((3, 5, 10, "0.5", 39, "-"), WS, "workspace of 39 bytes, n_rows=10 needs 40"),
    ((3, 5, 10, "0.5", 0, "-"), WS, "workspace of 0 bytes"),
    # precedence: the shape, the merges against the rows, the threshold, the pointers, the alignment, the size
    ((0, 11, 10, "nan", 0, "terwm"), ARG, "n_groups=0"),
    ((3, 11, 10, "nan", 0, "terwm"), ARG, "exceeds n_rows"),
    ((3, 5, 10, "nan", 0, "terwm"), ARG, "cos_thr is not"),
    ((3, 5, 10, "0.5", 0, "tm"), ARG, "null pointer"),
    ((3, 5, 10, "0.5", 0, "wm"), ARG, "null pointer"),
    ((3, 5, 10, "0.5", 0, "m"), ARG, "workspace is not"),
]
ACCEPTED = [
    ((1, 0, 0, "0.5", -1, "erwm"), 0),                                  # no rows: neither the merges, the labels nor the workspace are looked at
    ((3, 0, 10, "0.5", -1, "e"), 40),                                   # no merges: lo, hi and key may be null
    ((3, 9, 10, "-inf", -1, "-"), 40),
    ((3, 10, 10, "inf", 4000, "-"), 40),
    ((16, 121728, 121744, "0.3", -1, "-"), 4 * 121744),
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
    assert pure("size:10:3", "size:0:1", "size:-1:1", "size:10:0") == ["40", "0", "0", "0"]


def _entry(lib, n_groups, n_merges, n_rows, thr, ws_bytes, flags):
    """The same description through the built library: fake non-null pointers, nothing can be launched before the check has passed."""
    if ws_bytes < 0:
        ws_bytes = int(lib.sd_ahc_cut_workspace_bytes(n_rows, n_groups))
    merge = None if "e" in flags else 0x1000
    table = None if "t" in flags else 0x4000
    return lib.sd_ahc_cut_grouped(merge, 0x2000, 0x3000, table, 0x5000, n_groups, n_merges, n_rows, float(thr), 0x6000, 0x7000,
                                  None if "r" in flags else 0x8000, 0x9000, 0xA000, None if "w" in flags else 0xB004 if "m" in flags else 0xB000,
                                  ws_bytes, None)


def test_the_entry_is_wired_to_the_check():
    """Every refusal comes back from the entry with the same code and text, before anything is launched (a launch on this pointer soup
    would have returned SD_ERR_HIP here and faulted on a GPU)."""
    lib = N.load()
    for args, code, text in REFUSALS:
        refused(_entry(lib, *args), code, text)
        assert N.last_error().startswith(ENTRY + ": ")
    names = ("lo", "hi", "key", "first_merge", "first_row", "min_clusters", "max_clusters", "labels", "clusters", "bad", "ws")
    for name in names:
        p = {k: 0x1000 * (i + 1) for i, k in enumerate(names)}
        p[name] = None
        refused(lib.sd_ahc_cut_grouped(p["lo"], p["hi"], p["key"], p["first_merge"], p["first_row"], 3, 5, 10, 0.5, p["min_clusters"], p["max_clusters"],
                                       p["labels"], p["clusters"], p["bad"], p["ws"], 40, None), ARG, "null pointer")


def test_workspace_formula():
    """`parent`, one int32 per row, is the only state outside LDS: 4 n_rows bytes whatever the recordings' sizes."""
    size = N.load().sd_ahc_cut_workspace_bytes
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_cut.h").read()
    assert "sd_ahc_cut_workspace_bytes(n_rows, n_groups) = 4 n_rows" in header
    for rows, groups in ((0, 1), (1, 1), (7, 3), (128000, 256), (204800, 1024), (121744, 16), (2 ** 31 - 1, 5)):
        assert int(size(rows, groups)) == 4 * rows, (rows, groups)
    for rows, groups in ((10, 0), (10, -1), (-1, 3)):
        assert int(size(rows, groups)) == 0, (rows, groups)


# ------------------------------------------------------------------ the numpy statement

def test_the_statement_on_hand_made_logs():
    # rows 0 .. 4; merges (0,1) 0.9, (2,3) 0.8, (0,2) 0.5, (0,4) 0.2
    lo, hi, key = np.array([0, 2, 0, 0]), np.array([1, 3, 2, 4]), np.array([0.9, 0.8, 0.5, 0.2], np.float32)
    cut = lambda thr, a, b: CR.cut_one(lo, hi, key, 5, thr, a, b)  # noqa: E731
    assert cut(0.6, 1, 5)[0].tolist() == [0, 0, 1, 1, 2] and cut(0.6, 1, 5)[1:] == (3, 0)              # the threshold alone
    assert cut(0.5, 1, 5)[0].tolist() == [0, 0, 1, 1, 2]                                               # strict: a key at the threshold is not applied
    assert cut(0.6, 1, 2)[0].tolist() == [0, 0, 0, 0, 1]                                               # the maximum binds
    assert cut(0.6, 4, 5)[0].tolist() == [0, 0, 1, 2, 3]                                               # the minimum binds
    assert cut(-1.0, 1, 5)[0].tolist() == [0] * 5 and cut(2.0, 1, 9)[0].tolist() == [0, 1, 2, 3, 4]
    assert cut(0.6, 9, 9)[1:] == (5, 0)                                                                 # a minimum above n: nothing is applied
    # equal keys: the position decides, so the child (earlier) goes first
    assert CR.cut_one([0, 0], [1, 2], np.array([0.5, 0.5], np.float32), 3, 0.9, 2, 2)[0].tolist() == [0, 0, 1]
    # an empty log under a maximum it cannot reach is bad; without one it is n singletons
    assert CR.cut_one([], [], np.zeros(0, np.float32), 3, 0.5, 1, 2)[2] == 1
    assert CR.cut_one([], [], np.zeros(0, np.float32), 3, 0.5, 1, 3)[0].tolist() == [0, 1, 2]
    for broken in (dict(lo=[1], hi=[1]), dict(lo=[2], hi=[1]), dict(lo=[-1], hi=[1]), dict(lo=[0], hi=[3]), dict(key=[np.nan]), dict(key=[np.inf]),
                   dict(lo_bound=0), dict(lo_bound=3, hi_bound=2), dict(lo=[0, 0, 1], hi=[1, 2, 2], key=[0.5, 0.4, 0.3])):
        args = dict(lo=[0], hi=[1], key=[0.5], n=3, cos_thr=0.0, lo_bound=1, hi_bound=3)
        args.update(broken)
        labels, clusters, bad = CR.cut_one(**args)
        assert bad == 1 and clusters == 0 and labels.tolist() == [-1] * 3, broken
    # two parents for one row
    assert CR.cut_one([0, 1], [2, 2], np.array([0.5, 0.4], np.float32), 3, 0.0, 1, 3)[2] == 1
    assert CR.cut_one([0, 0], [2, 2], np.array([0.5, 0.4], np.float32), 3, 0.0, 1, 3)[2] == 0


def test_the_statement_equals_scipy_on_the_synthetic_logs():
    """Every full log of the GPU file as a linkage matrix (`log_linkage`): the cut into k is `fcluster(Z, k, "maxclust")`."""
    for equal_keys in (False, True):
        for n in sorted(set(CR.SIZES)) + [5000]:
            if n < 2:
                continue
            lo, hi, key = CR.random_log(n, 0, equal_keys=equal_keys)
            assert (lo < hi).all() and len(key) == n - 1
            Z = CR.log_linkage(lo, hi, key, n)
            thr = float(np.sort(key)[len(key) // 2])                    # exactly a key: the strict comparison
            c = int((key > np.float32(thr)).sum())
            for lo_b, hi_b in ((1, n), (1, max(1, (n - c) // 2)), (n - c + 3, CR.I32_MAX), (min(4, n), min(4, n))):
                labels, clusters, bad = CR.cut_one(lo, hi, key, n, thr, lo_b, hi_b)
                k = min(max(n - c, min(lo_b, n)), min(hi_b, n))
                assert bad == 0 and clusters == k == int(labels.max()) + 1, (n, lo_b, hi_b)
                assert np.array_equal(labels, CR.oracle_labels(Z, k)), (n, equal_keys, lo_b, hi_b)


def test_the_grouped_statement_and_the_promises():
    sizes = list(CR.SIZES)
    logs = [CR.random_log(n, 1, full=i % 2 == 0) for i, n in enumerate(sizes)]
    lo, hi, key, fm, fr = CR.pack(logs, sizes)
    lo_b, hi_b = CR.bounds_cases(sizes, logs, 0.25)["free"]
    labels, clusters, bad = CR.cut_numpy(lo, hi, key, fm, fr, 0.25, lo_b, hi_b)
    assert not bad.any() and clusters.sum() == int(sum(lab.max() + 1 for lab in np.split(labels, fr[1:-1]) if len(lab)))
    for g, n in enumerate(sizes):
        want = CR.cut_one(*logs[g], n, 0.25, lo_b[g], hi_b[g])
        assert np.array_equal(labels[fr[g]:fr[g + 1]], want[0]) and clusters[g] == want[1]
    broken = fm.copy()
    broken[3] = broken[4] + 1
    labels, clusters, bad = CR.cut_numpy(lo, hi, key, broken, fr, 0.25, lo_b, hi_b)
    assert bad.all() and (labels == -1).all() and not clusters.any()


def test_the_gaps_of_the_families():
    """The smallest difference of the two heights on either side of the cut, over k = 2 .. 12, from the oracle alone: only (1000 rows,
    k = 6) lies under the bar of 1e-4 the GPU test leaves a pair out at (an f32 score of a 192-wide sum is within 2.3e-5 of f64)."""
    want = {400: (4.7e-4, 11), 700: (3.3e-4, 10), 1000: (3.0e-5, 6)}
    under = []
    for family, (gap, at) in want.items():
        Z = CR.family_linkage(family)
        gaps = {k: CR.cut_gap(Z, k) for k in range(2, 13)}
        k = min(gaps, key=gaps.get)
        assert k == at and abs(gaps[k] - gap) < 0.05 * gap, (family, k, gaps[k])
        under += [(family, k) for k, v in gaps.items() if v < CR.GAP_BAR]
        assert CR.cut_gap(Z, 1) == float("inf")
    assert under == [(1000, 6)]
    assert CR.threshold_clusters(CR.family_linkage(700), 0.3) == 294 and CR.threshold_clusters(CR.family_linkage(1000), 0.3) == 671
    assert all(CR.threshold_clusters(CR.family_linkage(400), thr) == 2 for thr in (0.3, 0.1, 0.0))


# ------------------------------------------------------------------ the drivers on the CPU

def _groups(recs, thr, operator, **kw):
    X = torch.from_numpy(np.concatenate([x for _, x in recs]))
    return ahc_gpu.ahc_cosine_groups(X, [len(x) for _, x in recs], thr, operator=operator, return_info=True, **kw)


@pytest.mark.parametrize("thr", AG.DRIVER_THRESHOLDS)
def test_bounds_that_do_not_bind_change_nothing(thr):
    """min = 1, max = n: the labels of the unbounded driver on every recording, in exactly its nearest passes (phase A is today's loop
    and phase B does not run)."""
    recs = AG.driver_recordings(thr)
    plain, bounded = AG.NumpyGroupedSums(), CR.NumpyCutSums()
    want, winfo = _groups(recs, thr, plain)
    got, info = _groups(recs, thr, bounded, min_clusters=1, max_clusters=[max(len(x), 1) for _, x in recs])
    assert bounded.passes == plain.passes and bounded.cut_calls == 1
    assert all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))
    assert info["rounds"] == winfo["rounds"] and info["clusters"] == winfo["clusters"] == info["threshold_clusters"] and info["rounds_full"] == 0
    assert info["gram_tiles"] == winfo["gram_tiles"]
    lo, hi, key, first_merge, first_row = bounded.seen[:5]
    assert (lo < hi).all() and np.isfinite(key).all() and (key > np.float32(thr)).all()
    assert first_row.tolist() == np.concatenate([[0], np.cumsum([len(x) for _, x in recs])]).tolist() and first_merge[-1] == len(key)
    # alone, through the rows driver with the ungrouped nearest: the same labels
    for (f, x), w in zip(recs, want):
        alone = ahc_gpu.ahc_cosine_rows(torch.from_numpy(x), thr, operator=CR.NumpyCutSums(), min_clusters=1, max_clusters=max(len(x), 1))
        assert np.array_equal(alone, w), f


@pytest.mark.parametrize("case", CR.DRIVER_CASES)
def test_binding_bounds_equal_the_oracle(case):
    """Every driver case of the GPU file through the numpy operator: k = 1 .. 12 as min = max, and the (min, max) cases."""
    thr, lo_b, hi_b = case
    recs = CR.driver_recordings()
    op = CR.NumpyCutSums()
    labels, info = _groups(recs, thr, op, min_clusters=lo_b, max_clusters=hi_b)
    skipped = CR.check_driver_case(labels, case, recs)
    assert set(skipped) <= {(1000, 6)}, skipped
    fams = [f for f, _ in recs]
    if thr == 0.3:
        assert [info["threshold_clusters"][fams.index(f)] for f in (400, 700, 1000)] == [2, 294, 671]
        assert (info["rounds_full"] > 0) == (hi_b < 294)
    lo, hi, key, first_merge, _ = op.seen[:5]
    for g in range(len(recs)):                                          # the keys of a recording are monotone: none exceeds an earlier key of its lo or hi
        a, b = first_merge[g], first_merge[g + 1]
        height = {}
        for x, y, k in zip(lo[a:b], hi[a:b], key[a:b]):
            assert k <= height.get(x, np.inf) and k <= height.get(y, np.inf)
            height[x] = k
        if info["threshold_clusters"][g] > hi_b:
            assert b - a == len(recs[g][1]) - 1                        # the complete dendrogram


def test_stopping_at_the_maximum_would_be_wrong():
    """The six clusters of DESIGN section 22 under max = 4 at a threshold above every score.  The first round merges (A, B) at 0.5 and
    (C, D) at 0.1 and reaches 4 clusters; the second-highest merge of the dendrogram, (AB, E) at 0.3, is made in the next round."""
    X = torch.from_numpy(CR.counter_example())
    want = CR.oracle_labels(CR.host_linkage(X.numpy()), 4)
    assert want.tolist() == [0, 0, 1, 2, 0, 3]
    op = CR.NumpyCutSums()
    got, info = ahc_gpu.ahc_cosine_rows(X, 0.7, operator=op, min_clusters=1, max_clusters=4, return_info=True)
    assert got.tolist() == want.tolist() and info["threshold_clusters"] == 6 and info["clusters"] == 4 and info["rounds_full"] >= 2
    lo, hi, key = op.seen[:3]
    assert list(zip(lo[:3].tolist(), hi[:3].tolist())) == [(0, 1), (2, 3), (0, 4)] and np.allclose(key[:3], [0.5, 0.1, 0.3], atol=1e-6)
    assert len(key) == 5                                                # the complete dendrogram

    class StopsEarly(CR.NumpyCutSums):
        """Phase B ends as soon as no more than 4 clusters are left."""

        def merge(self, sums, count, inv_count, nn, best, cos_thr):
            if cos_thr == float("-inf") and sums.shape[0] <= 4:
                return torch.arange(sums.shape[0], dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
            return super().merge(sums, count, inv_count, nn, best, cos_thr)
    early = ahc_gpu.ahc_cosine_rows(X, 0.7, operator=StopsEarly(), min_clusters=1, max_clusters=4)
    assert early.tolist() == [0, 0, 1, 1, 2, 3] and early.tolist() != want.tolist()


def test_refusals_and_defaults():
    X = torch.from_numpy(A.family_rows(400)[0][:50])

    class NoLaunch(CR.NumpyCutSums):
        def normalise(self, X):
            raise AssertionError("the operator was reached")
    for kw, text in ((dict(min_clusters=3, max_clusters=2), "min_clusters=3 max_clusters=2"), (dict(min_clusters=0), "min_clusters=0"),
                     (dict(min_clusters=0, max_clusters=4), "min_clusters=0"), (dict(max_clusters=0), "max_clusters=0")):
        with pytest.raises(ValueError, match=text):
            ahc_gpu.ahc_cosine_rows(X, 0.3, operator=NoLaunch(), **kw)
        with pytest.raises(ValueError, match=text):
            ahc_gpu.ahc_cosine_groups(X, [20, 30], 0.3, operator=NoLaunch(), **kw)
        with pytest.raises(ValueError, match=text):
            ahc_gpu.AhcGpuClusterer(0.3, **kw)
    with pytest.raises(ValueError, match=r"recording 1: .*min_clusters=5 max_clusters=4"):
        ahc_gpu.ahc_cosine_groups(X, [20, 30], 0.3, operator=NoLaunch(), min_clusters=[1, 5], max_clusters=4)
    with pytest.raises(ValueError, match="max_clusters has 3 entries for 2 recordings"):
        ahc_gpu.ahc_cosine_groups(X, [20, 30], 0.3, operator=NoLaunch(), max_clusters=[4, 4, 4])
    with pytest.raises(TypeError, match="need an operator with cut"):
        ahc_gpu.ahc_cosine_groups(X, [20, 30], 0.3, operator=AG.NumpyGroupedSums(), max_clusters=4)
    # a bad verdict of the cut names the recording

    class Breaks(CR.NumpyCutSums):
        def cut(self, lo, hi, key, first_merge, *rest):
            hi = hi.clone()
            hi[int(first_merge[1])] = 0
            return super().cut(lo, hi, key, first_merge, *rest)
    with pytest.raises(RuntimeError, match=r"recording\(s\) \[1\]"):
        ahc_gpu.ahc_cosine_groups(X, [20, 30], 0.3, operator=Breaks(), max_clusters=4)
    # the clusterer and its factory pass the bounds on
    made = ahc_gpu.AhcGpuClusterer.factory(0.3, operator=CR.NumpyCutSums(), min_clusters=3, max_clusters=3)(metric="euclidean")
    assert (made.min_clusters, made.max_clusters) == (3, 3) and int(made.fit_predict(X.numpy()).max()) == 2
    plain = ahc_gpu.AhcGpuClusterer.factory(0.3)()
    assert plain.min_clusters is None and plain.max_clusters is None
    for fn in (ahc_gpu.ahc_cosine_rows, ahc_gpu.ahc_cosine_groups, ahc_gpu.AhcGpuClusterer.__init__, ahc_gpu.AhcGpuClusterer.factory):
        params = inspect.signature(fn).parameters
        assert params["min_clusters"].default is None and params["max_clusters"].default is None, fn
    assert "cut(lo, hi, key, first_merge, first_row, cos_thr, min_clusters, max_clusters)" in ahc_gpu.__doc__
    lo = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ahc_cut_grouped(lo, lo, torch.zeros(3), torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 4], dtype=torch.int32), 0.5,
                            lo[:1], lo[:1])


def test_speaker_bounds_is_off_by_default_and_needs_ahc_gpu(tmp_path):
    for fn in (db.diarize_audio, db.diarize_audios, db.Diarizer.__init__):
        param = inspect.signature(fn).parameters["speaker_bounds"]
        assert param.default is False, fn
    assert inspect.signature(db.diarize_audio).parameters["speaker_bounds"].kind is inspect.Parameter.KEYWORD_ONLY
    tool = open(os.path.join(os.path.dirname(HERE), "tools", "diarize_sharded.py")).read()
    assert re.search(r'add_argument\("--speaker-bounds", action="store_true"', tool) and "speaker_bounds=a.speaker_bounds" in tool
    audio = {"waveform": np.zeros(16000, np.float32), "sample_rate": 16000}
    for clustering in ("spectral", "spectral_gpu", "ahc"):
        with pytest.raises(ValueError, match="speaker_bounds=True bounds the cluster count of clustering='ahc_gpu'"):
            db.diarize_audio(audio, 0.35, 0.1, 2, 6, clustering=clustering, speaker_bounds=True, encoder=lambda w: None)
        with pytest.raises(ValueError, match="speaker_bounds=True"):
            db.Diarizer(db.DiarizationParameters(), clustering=clustering, speaker_bounds=True)
    with pytest.raises(ValueError, match="ahc_gpu"):
        db.diarize_audios([audio], 0.35, 0.1, 2, 6, clustering="spectral", speaker_bounds=True)
    assert db.Diarizer(db.DiarizationParameters(), clustering="ahc_gpu", speaker_bounds=True).speaker_bounds is True
    assert db.Diarizer(db.DiarizationParameters()).speaker_bounds is False
    # what reaches the driver: each bound clamped to the number of windows
    assert db._cluster_bounds(False, 2, 6, [10, 3]) == {}
    assert db._cluster_bounds(True, 2, 6, [10, 3, 1, 0]) == {"min_clusters": [2, 2, 1, 1], "max_clusters": [6, 3, 1, 1]}
    assert db._cluster_bounds(True, 4, 4, [3], one=True) == {"min_clusters": 3, "max_clusters": 3}
    for lo_b, hi_b in ((0, 6), (5, 4)):
        with pytest.raises(ValueError, match="1 <= min_speakers <= max_speakers"):
            db._cluster_bounds(True, lo_b, hi_b, [10])
