"""No-GPU checks of the device k-means (include/sd_hip_kmeans.h: sd_kmeans_grouped_f64, speech-diarization_amd/csrc/kmeans/,
`kmeans_gpu.k_means_rows / k_means_groups`, `cluster_gpu.spectral(..., assign_labels="device")`, clustering="spectral_device"): the
header and its binding table, the untouched versions and tables, the census of the new source directory, the pure check
(csrc/kmeans/sd_kmeans_check.h, built alone with sanitizers) with its codes and precedence, the workspace formula, the draws against
scikit-learn's generator, the numpy statement of the entry against `sklearn.cluster.k_means` (exactly, under a margin condition on
the inputs), and the drivers run on the CPU through the statement as their `launch`."""
import inspect
import os
import re
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import kmeans_ref as KR  # noqa: E402
import launch_log as L  # noqa: E402
import spectral_ref as R  # noqa: E402
from abi_rules import ARG, WS, check_header_and_table, check_versions, refused  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import cluster_gpu, kmeans_gpu, ops  # noqa: E402
from speech_diarization_amd import diarization_baseline as db  # noqa: E402

CSRC = N.PKG_DIR / "csrc"
KMEANS = CSRC / "kmeans"
NAMES = {"sd_kmeans_abi_version", "sd_kmeans_grouped_workspace_bytes", "sd_kmeans_grouped_f64"}
ENTRY = "sd_kmeans_grouped_f64"
KERNELS = {"kmeans_lloyd_kernel", "kmeans_select_kernel"}


# ------------------------------------------------------------------ ABI

def test_header_and_binding_table_name_the_same_exported_entries():
    others = (N.PROTOTYPES, N.SPECTRAL_PROTOTYPES, N.AHC_PROTOTYPES, N.HDBSCAN_PROTOTYPES, N.DIAG_PROTOTYPES, N.TRACE_PROTOTYPES, N.TREE_ENTRIES,
              N.CUT_ENTRIES)
    assert check_header_and_table("sd_hip_kmeans.h", N.KMEANS_ENTRIES, others) == NAMES
    # `ops.launch` takes them from a set of their own; the older sets stay what they were
    assert ops._LAUNCHABLE == ops._ENTRIES | set(N.TREE_ENTRIES) and ops._CUT_LAUNCHABLE == set(N.CUT_ENTRIES)
    assert ops._KMEANS_LAUNCHABLE == NAMES and not NAMES & (ops._LAUNCHABLE | ops._CUT_LAUNCHABLE)
    assert '("sd_hip_kmeans.h", KMEANS_ENTRIES, "sd_kmeans_abi_version", SD_KMEANS_ABI_VERSION, "k-means ")' in open(N.__file__).read()
    with pytest.raises(ValueError, match="not an entry"):
        ops.launch("sd_kmeans_grouped", torch.zeros(1))


def test_the_new_version_is_one_and_every_other_is_untouched():
    assert N.SD_KMEANS_ABI_VERSION == 1
    check_versions(sd_kmeans_abi_version=1, sd_cut_abi_version=1, sd_tree_abi_version=1, sd_abi_version=11, sd_spectral_abi_version=1,
                   sd_ahc_abi_version=1, sd_hdbscan_abi_version=1, sd_diag_abi_version=1, sd_trace_abi_version=3)
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_kmeans.h").read()
    assert re.search(r"#define\s+SD_KMEANS_ABI_VERSION\s+1\b", header)
    for name, value in (("EMPTY", KR.EMPTY), ("NONFINITE", KR.NONFINITE), ("BAD_K", KR.BAD_K), ("BAD_DRAW", KR.BAD_DRAW),
                        ("BAD_PROMISE", KR.BAD_PROMISE), ("MAX_K", KR.MAX_K), ("MAX_DIM", KR.MAX_DIM), ("MAX_INIT", KR.MAX_INIT),
                        ("U_STRIDE", KR.U_CENTRES * KR.U_TRIALS)):
        assert re.search(rf"#define\s+SD_KMEANS_{name}\s+{value}\b", header), name
    assert (kmeans_gpu.EMPTY, kmeans_gpu.NONFINITE, kmeans_gpu.BAD_K, kmeans_gpu.BAD_DRAW, kmeans_gpu.BAD_PROMISE) == \
        (KR.EMPTY, KR.NONFINITE, KR.BAD_K, KR.BAD_DRAW, KR.BAD_PROMISE)
    assert (kmeans_gpu.U_CENTRES, kmeans_gpu.U_TRIALS, N.SD_KMEANS_U_STRIDE) == (KR.U_CENTRES, KR.U_TRIALS, 155)


# ------------------------------------------------------------------ the census of the directory

def test_the_directory_has_two_kernels_with_labelled_launches():
    srcs = {f.name: f.read_text() for f in sorted(KMEANS.glob("*"))}
    assert sorted(srcs) == ["sd_kmeans.hip", "sd_kmeans_check.h"]
    text = srcs["sd_kmeans.hip"]
    kernels = re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", text)
    assert set(kernels) == KERNELS and len(kernels) == 2
    assert re.findall(r'\bSD_CHECK_LAUNCH\("([a-z0-9_]+)"\)', text) == ["kmeans_lloyd_kernel", "kmeans_select_kernel"]
    assert len(re.findall(r"\bhipLaunchKernelGGL\(", text)) == 2
    code = re.sub(r"//.*", "", text)
    # integer atomics on LDS only: every atomic is on a __shared__ int array
    atomics = re.findall(r"\batomic\w*\(&(\w+)", code)
    assert atomics and set(atomics) == {"s_trial", "s_cnt", "s_map"} and len(atomics) == len(re.findall(r"atomic", code)), atomics
    for name in set(atomics):
        assert re.search(rf"__shared__ int {name}\[", code), name
    assert "fast-math" not in code and "ffast" not in code and not re.search(r"atomic\w*\([^)]*(float|double)", code)
    assert "__fdividef" not in code and "__frcp" not in code
    # the entry refuses through the one pure check and has no argument check of its own
    assert not re.search(r"\bSD_CHECK_ARG\(", code) and len(re.findall(r"\bsd_kmeans_check\(", code)) == 1
    assert len(re.findall(r"\bsd_set_error\(", code)) == 1 and len(re.findall(r"\bsd_kmeans_workspace_bytes\(", code)) == 1
    # outside the census of csrc/*.hip and of the other directories
    import kernel_census
    assert not KERNELS & {L.kernel_of(lb) for lb in kernel_census.KERNEL_TESTS}
    for other in ("ahc", "cut", "diag", "hdbscan", "tree"):
        theirs = "".join(f.read_text() for f in sorted((CSRC / other).glob("*")))
        assert not KERNELS & set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", theirs))
    for f in CSRC.glob("*.hip"):
        assert not any(k in f.read_text() for k in KERNELS), f.name
    # the check is pure: no HIP, nothing but the status codes
    raw = srcs["sd_kmeans_check.h"]
    assert re.findall(r'#include [<"]([^>"]+)[>"]', raw) == ["stdio.h", "sd_hip.h"] and "hip" not in re.sub(r"//.*|sd_hip\.h", "", raw).lower()


def test_the_labels_are_asserted_by_the_gpu_tests():
    text = open(os.path.join(HERE, "test_gpu_kmeans.py")).read()
    assert "pytestmark = pytest.mark.gpu" in text
    assert 'KERNELS = {"kmeans_lloyd_kernel", "kmeans_select_kernel"}' in text
    bodies = re.findall(r"^def test_\w+\(.*?(?=^def |^class |^@|\Z)", text, flags=re.M | re.S)
    # every test launches under the log: itself, or through _launch / _twice, which do
    assert len(bodies) >= 6 and all(any(via in b for via in ("expect_launches", "_launch(", "_twice(")) for b in bodies)
    assert "expect_launches(exactly=KERNELS)" in re.search(r"^def _launch\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0)
    assert "_launch(" in re.search(r"^def _twice\(.*?(?=^def |^@|\Z)", text, flags=re.M | re.S).group(0)


def test_build_list_and_fingerprint_cover_the_directory():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sd_build_native_kmeans", str(N.PKG_DIR / "build_native.py"))
    bn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bn)
    assert "kmeans/sd_kmeans.hip" in bn.SOURCES and all((bn.CSRC / s).exists() for s in bn.SOURCES)
    assert len({os.path.basename(s) for s in bn.SOURCES}) == len(bn.SOURCES)
    assert '(CSRC / "kmeans").glob("*")' in (N.PKG_DIR / "build_native.py").read_text()


# ------------------------------------------------------------------ the pure check

@pytest.fixture(scope="module")
def pure(tmp_path_factory):
    cxx = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(cxx), "no clang++ on this machine"
    exe = tmp_path_factory.mktemp("kmeans_check") / "kmeans_check_pure"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           f"-I{N.PKG_DIR.parent / 'include'}", os.path.join(HERE, "helpers", "kmeans_check_pure.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(*calls):
        ran = subprocess.run([str(exe), *calls], capture_output=True, text=True)
        assert ran.returncode == 0 and not ran.stderr, (ran.returncode, ran.stderr[-2000:])
        return ran.stdout.splitlines()
    return run


# (n_rows, dim, ld, n_groups, n_init, max_iter, max_k, max_rows, tol_rel, ws_bytes (-1: the need), flags) -> (status, text in the message)
GOOD = (1000, 8, 8, 3, 10, 300, 8, 500, "1e-4", -1, "-")


def _with(**kw):
    names = ("n_rows", "dim", "ld", "n_groups", "n_init", "max_iter", "max_k", "max_rows", "tol_rel", "ws_bytes", "flags")
    return tuple(kw.get(name, value) for name, value in zip(names, GOOD))


REFUSALS = [
    (_with(n_groups=0), ARG, "n_groups=0 n_rows=1000"),
    (_with(n_groups=-3), ARG, "n_groups=-3"),
    (_with(n_rows=-1), ARG, "n_rows=-1"),
    (_with(n_init=0), ARG, "n_init=0 outside [1, 16]"),
    (_with(n_init=17), ARG, "n_init=17 outside [1, 16]"),
    (_with(dim=0), ARG, "dim=0 outside [1, 32]"),
    (_with(dim=33, ld=33), ARG, "dim=33 outside [1, 32]"),
    (_with(ld=7), ARG, "ld=7 is less than dim=8"),
    (_with(max_iter=0), ARG, "max_iter=0"),
    (_with(max_k=1), ARG, "max_k=1 outside [2, 32]"),
    (_with(max_k=33), ARG, "max_k=33 outside [2, 32]"),
    (_with(max_rows=0), ARG, "max_rows=0"),
    (_with(tol_rel="-1e-9"), ARG, "tol_rel is negative or not finite"),
    (_with(tol_rel="nan"), ARG, "tol_rel is negative or not finite"),
    (_with(tol_rel="inf"), ARG, "tol_rel is negative or not finite"),
    (_with(flags="t"), ARG, "null pointer"),
    (_with(flags="r"), ARG, "null pointer"),
    (_with(flags="a"), ARG, "rows are not 8-byte aligned"),
    (_with(flags="m"), ARG, "workspace is not 16-byte aligned"),
    (_with(ws_bytes=120479), WS, "workspace of 120479 bytes, n_rows=1000 n_groups=3 n_init=10 needs 120480"),
    (_with(ws_bytes=0), WS, "workspace of 0 bytes"),
    # precedence: the groups and rows, the restarts, the shape, the iterations, the bounds, the tolerance, the pointers, the alignments, the size
    (_with(n_groups=0, n_init=0, dim=0, tol_rel="nan", ws_bytes=0, flags="tram"), ARG, "n_groups=0"),
    (_with(n_init=0, dim=0, tol_rel="nan", ws_bytes=0, flags="tram"), ARG, "n_init=0"),
    (_with(dim=0, ld=-1, max_iter=0, tol_rel="nan", ws_bytes=0, flags="tram"), ARG, "dim=0"),
    (_with(ld=1, max_iter=0, max_k=0, tol_rel="nan", ws_bytes=0, flags="tram"), ARG, "ld=1"),
    (_with(max_iter=0, max_k=0, max_rows=0, tol_rel="nan", ws_bytes=0, flags="tram"), ARG, "max_iter=0"),
    (_with(max_k=0, max_rows=0, tol_rel="nan", ws_bytes=0, flags="tram"), ARG, "max_k=0"),
    (_with(max_rows=0, tol_rel="nan", ws_bytes=0, flags="tram"), ARG, "max_rows=0"),
    (_with(tol_rel="nan", ws_bytes=0, flags="tram"), ARG, "tol_rel"),
    (_with(ws_bytes=0, flags="ram"), ARG, "null pointer"),
    (_with(ws_bytes=0, flags="am"), ARG, "rows are not"),
    (_with(ws_bytes=0, flags="m"), ARG, "workspace is not"),
]
ACCEPTED = [
    (GOOD, 12 * 10 * 1000 + 16 * 10 * 3),
    (_with(n_rows=0, flags="ra"), 16 * 10 * 3),                         # no rows: neither the rows nor the labels are looked at
    (_with(tol_rel="0"), 120480),
    (_with(dim=1, ld=1, max_k=32, n_init=16, max_iter=1, max_rows=1), 12 * 16 * 1000 + 16 * 16 * 3),
    (_with(dim=32, ld=40, max_k=2, n_init=1, ws_bytes=10 ** 6), 12 * 1000 + 16 * 3),
    (_with(n_rows=121744, n_groups=16), 12 * 10 * 121744 + 16 * 10 * 16),
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
    assert pure("size:1000:3:10", "size:0:1:1", "size:-1:1:1", "size:10:0:1", "size:10:1:0", "size:10:1:17") == \
        ["120480", "16", "0", "0", "0", "0"]


def test_the_lds_layout(pure):
    """The doubles before the rows (centres, the partial sums of 256 / dim row slices, means, five candidates) and the doubles the
    rows may take: dim (max_rows | 1) when that fits into 160 KB less 1 KB of static words, 0 (streamed) when it does not."""
    room = (160 * 1024 - 1024) // 8
    for dim, max_k, max_rows in ((1, 2, 3), (1, 32, 1000), (4, 4, 500), (8, 8, 7609), (8, 8, 2600), (32, 32, 700), (32, 32, 300), (31, 21, 257),
                                 (12, 12, 50000), (5, 7, 2147483647)):
        fixed = max_k * dim + (256 // dim) * max_k * dim + dim + 5 * dim
        want = dim * (max_rows | 1)
        assert pure(f"lds:{dim}:{max_k}:{max_rows}") == [f"{fixed} {want if want <= room - fixed else 0}"], (dim, max_k, max_rows)
    # the streamed recordings of the GPU test do not fit, the folder shapes of the project do
    assert pure("lds:8:8:2600", "lds:32:32:700", "lds:4:4:500", "lds:8:8:200")[0].endswith(" 0")
    assert [ln.split()[1] for ln in pure("lds:8:8:2600", "lds:32:32:700", "lds:4:4:500", "lds:4:4:200")] == ["0", "0", "2004", "804"]


def _entry(lib, n_rows, dim, ld, n_groups, n_init, max_iter, max_k, max_rows, tol, ws_bytes, flags):
    """The same description through the built library: fake non-null pointers, nothing can be launched before the check has passed."""
    if ws_bytes < 0:
        ws_bytes = int(lib.sd_kmeans_grouped_workspace_bytes(n_rows, n_groups, n_init))
    rows = None if "r" in flags else 0x1004 if "a" in flags else 0x1000
    return lib.sd_kmeans_grouped_f64(rows, ld, n_rows, dim, None if "t" in flags else 0x2000, n_groups, 0x3000, n_init, max_iter, float(tol), max_k,
                                     max_rows, 0x4000, 0x5000, 0x6000, 0x7000, 0x8000, 0x9000, 0xA000, 0xB004 if "m" in flags else 0xB000, ws_bytes,
                                     None)


def test_the_entry_is_wired_to_the_check():
    """Every refusal comes back from the entry with the same code and text, before anything is launched (a launch on this pointer soup
    would have returned SD_ERR_HIP here and faulted on a GPU)."""
    lib = N.load()
    for args, code, text in REFUSALS:
        refused(_entry(lib, *args), code, text)
        assert N.last_error().startswith(ENTRY + ": ")
    names = ("rows", "first_row", "k", "first", "u", "labels", "chosen", "inertia", "iters", "flags", "ws")
    for name in names:
        p = {k: 0x1000 * (i + 1) for i, k in enumerate(names)}
        p[name] = None
        refused(lib.sd_kmeans_grouped_f64(p["rows"], 8, 1000, 8, p["first_row"], 3, p["k"], 10, 300, 1e-4, 8, 500, p["first"], p["u"], p["labels"],
                                          p["chosen"], p["inertia"], p["iters"], p["flags"], p["ws"], 120480, None), ARG, "null pointer")


def test_workspace_formula():
    size = N.load().sd_kmeans_grouped_workspace_bytes
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_kmeans.h").read()
    assert "sd_kmeans_grouped_workspace_bytes(n_rows, n_groups, n_init) = 12 n_init n_rows + 16 n_init n_groups" in header
    for rows, groups, init in ((0, 1, 1), (1, 1, 1), (7, 3, 10), (128000, 256, 10), (204800, 1024, 10), (121744, 16, 16), (2 ** 31 - 1, 5, 16)):
        assert int(size(rows, groups, init)) == 12 * init * rows + 16 * init * groups, (rows, groups, init)
    for rows, groups, init in ((10, 0, 10), (10, -1, 10), (-1, 3, 10), (10, 3, 0), (10, 3, 17)):
        assert int(size(rows, groups, init)) == 0, (rows, groups, init)


# ------------------------------------------------------------------ the draws

@pytest.mark.parametrize("k", [2, 3, 7, 8, 20, 21, 32])
def test_the_draws_leave_the_generator_where_scikit_learn_leaves_it(k):
    """t = 2 + floor(ln k) is 2 at k = 2, 3 up to 7, 4 up to 20 and 5 from 21 on."""
    assert KR.trials_of(k) == {2: 2, 3: 3, 7: 3, 8: 4, 20: 4, 21: 5, 32: 5}[k]
    n = 3 * k + 5
    X = KR.blob(n, 3, k, 2.0, k)
    for n_init in (1, 10):
        ours, theirs = np.random.RandomState(k), np.random.RandomState(k)
        first, u = kmeans_gpu.kmeans_draws(ours, n, k, n_init)
        assert first.shape == (n_init,) and first.dtype == np.int32 and u.shape == (n_init, k - 1, KR.trials_of(k))
        assert ((0 <= first) & (first < n)).all() and ((0 <= u) & (u < 1)).all()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            KR.sklearn_labels(X, k, theirs, n_init=n_init)
        a, b = ours.get_state(), theirs.get_state()
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:], (k, n_init)


# ------------------------------------------------------------------ the statement against scikit-learn, exactly

def _both(X, k, rs_ours, rs_theirs, **kw):
    """(statement through the driver, scikit-learn, the launch with its trace); both generators end in the same state"""
    launch = KR.NumpyLaunch()
    got, info = kmeans_gpu.k_means_rows(X, k, rs_ours, return_info=True, launch=launch, **kw)
    want = KR.sklearn_labels(X, k, rs_theirs, **kw)
    assert np.array_equal(rs_ours.get_state()[1], rs_theirs.get_state()[1]) and rs_ours.get_state()[2] == rs_theirs.get_state()[2]
    return got, info, want, launch


def _check_exact(X, k, seed, advance=0, **kw):
    ours, theirs = np.random.RandomState(seed), np.random.RandomState(seed)
    if advance:
        ours.uniform(-1, 1, advance), theirs.uniform(-1, 1, advance)
    got, info, want, launch = _both(X, k, ours, theirs, **kw)
    margins = launch.trace.margins
    print(f"{X.shape} k={k} {kw}: iterations {min(launch.trace.iterations)}..{max(launch.trace.iterations)}, margins "
          + " ".join(f"{m}={v:.1e}" for m, v in margins.items()))
    # a condition on the INPUT, not a tolerance on anything computed: no comparison is decided by less than 1e-9 (relative)
    assert all(v >= KR.MARGIN_BAR for v in margins.values()), margins
    assert not info["fallback"] and got.dtype == np.int32
    assert np.array_equal(got, want[0]), f"{int((got != want[0]).sum())} of {len(got)} labels differ"
    assert info["iterations"] == want[2] and abs(info["inertia"] - want[1]) <= 1e-9 * want[1]
    return launch.trace


@pytest.mark.parametrize("n,k", KR.PLANTED)
def test_the_statement_on_spectral_embeddings(n, k):
    X, _ = R.planted_rows(n, k, 1.5, seed=0)        # noise 1.5: at 0.9 a cluster's rows nearly coincide and two candidates of a seeding step tie
    emb, _ = cluster_gpu.spectral_embedding(None, k, operator=R.NumpyOperator(R.cosine(X).astype(np.float32)))
    _check_exact(emb, k, 0, advance=n)


VARIANTS = ({}, {"max_iter": 3}, {"tol": 0})
_TRACES = {}


def _blob_trace(case, kw):
    """The exact comparison of one blob case under one variant, run once per process"""
    key = (case, tuple(sorted(kw.items())))
    if key not in _TRACES:
        _TRACES[key] = _check_exact(KR.blob(*case), case[2], case[4], **kw)
    return _TRACES[key]


@pytest.mark.parametrize("case", KR.BLOBS)
def test_the_statement_on_blobs(case):
    for kw in VARIANTS:
        _blob_trace(case, kw)
    if case[0] <= 300:
        for n_init in (1, 3):
            _check_exact(KR.blob(*case), case[2], case[4], n_init=n_init)


def test_every_branch_was_taken():
    """A strict stop, a tolerance stop, the iterations exhausted, a restart that displaces the incumbent, one refused as the same
    clustering at a lower inertia, one refused for its inertia: each at least once, counted by the statement over three of the runs
    above (tol = 0 runs in every blob case)."""
    total = {c: 0 for c in KR.COUNTERS}
    for case, kw in ((KR.BLOBS[8], {"max_iter": 3}), (KR.BLOBS[10], {}), (KR.BLOBS[0], {"tol": 0})):
        trace = _blob_trace(case, kw)
        for c in KR.COUNTERS:
            total[c] += trace.counters[c]
    assert all(total[c] > 0 for c in KR.COUNTERS), total


def test_the_statement_in_detail():
    # three obvious clusters on a line, one restart, the draws by hand: first centre row 0; u = 0.5 picks by the prefix sum of `closest`
    X = np.array([[0.0], [0.1], [10.0], [10.1], [20.0], [20.1]])
    u = np.zeros((1, KR.U_CENTRES, KR.U_TRIALS))
    u[0, 0, :3] = (0.1, 0.1, 0.1)          # closest = 0, .01, 100, 102.01, 400, 404.01: pot 1006.03, v = 100.6 -> 3 prefixes below -> row 3
    u[0, 1, :3] = (0.999, 0.999, 0.999)    # -> the last row
    one = KR.kmeans_one(X, 3, np.array([0]), u)
    assert one["labels"].tolist() == [0, 0, 1, 1, 2, 2] and one["flags"] == 0 and one["chosen"] == 0 and one["iters"] == 2
    assert abs(one["inertia"] - 0.015) < 1e-12
    for k, flag in ((1, KR.BAD_K), (6, KR.BAD_K), (33, KR.BAD_K)):
        assert KR.kmeans_one(X, k, np.array([0]), u)["flags"] == flag
    assert KR.kmeans_one(X, 3, np.array([6]), u)["flags"] == KR.BAD_DRAW and KR.kmeans_one(X, 3, np.array([-1]), u)["flags"] == KR.BAD_DRAW
    bad = X.copy()
    bad[4, 0] = np.inf
    assert KR.kmeans_one(bad, 3, np.array([0]), u)["flags"] == KR.NONFINITE
    assert (KR.kmeans_one(bad, 3, np.array([0]), u)["labels"] == -1).all()
    assert KR.same_clustering([0, 0, 1, 2], [2, 2, 0, 1], 3) and not KR.same_clustering([0, 0, 1, 2], [2, 1, 0, 1], 3)


# ------------------------------------------------------------------ the drivers on the CPU

def test_groups_equal_scikit_learn_per_recording_and_launch_once():
    cases = [KR.BLOBS[0], KR.BLOBS[7], KR.BLOBS[8], KR.BLOBS[9]]
    Xs = [KR.blob(*c) for c in cases]
    d = max(x.shape[1] for x in Xs)
    X = np.concatenate([np.pad(x, ((0, 0), (0, d - x.shape[1]))) for x in Xs])        # zero columns change no distance
    launch = KR.NumpyLaunch()
    states = [np.random.RandomState(c[4]) for c in cases]
    labels, info = kmeans_gpu.k_means_groups(X, [len(x) for x in Xs], [c[2] for c in cases], states, return_info=True, launch=launch)
    assert launch.calls == 1 and info["fallback"] == []
    for g, (c, x) in enumerate(zip(cases, Xs)):
        theirs = np.random.RandomState(c[4])
        want = KR.sklearn_labels(x, c[2], theirs)
        assert np.array_equal(labels[g], want[0]) and info["iterations"][g] == want[2], c
        assert np.array_equal(states[g].get_state()[1], theirs.get_state()[1])
    # one generator for all recordings: they draw from it in turn, as consecutive calls of scikit-learn would
    shared, theirs = np.random.RandomState(5), np.random.RandomState(5)
    labels = kmeans_gpu.k_means_groups(X, [len(x) for x in Xs], [c[2] for c in cases], shared, launch=KR.NumpyLaunch())
    for g, (c, x) in enumerate(zip(cases, Xs)):
        assert np.array_equal(labels[g], KR.sklearn_labels(x, c[2], theirs)[0]), c
    assert np.array_equal(shared.get_state()[1], theirs.get_state()[1])


def test_an_empty_cluster_falls_back_to_the_host():
    """40 rows of 3 distinct values at k = 5: the statement flags EMPTY, the driver returns scikit-learn's labels (which relocates) and
    names the recording; its neighbours in the launch keep their device labels."""
    deg = KR.degenerate_rows()
    one = KR.kmeans_one(deg, 5, *kmeans_gpu.kmeans_draws(np.random.RandomState(0), 40, 5, 10))
    assert one["flags"] == KR.EMPTY and (one["labels"] == -1).all()
    a, b = KR.blob(*KR.BLOBS[0]), KR.blob(*KR.BLOBS[9])[:, :2]
    X = np.concatenate([a, deg, b])
    ours, theirs = np.random.RandomState(3), np.random.RandomState(3)
    launch = KR.NumpyLaunch()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        labels, info = kmeans_gpu.k_means_groups(X, [len(a), 40, len(b)], [3, 5, 6], ours, return_info=True, launch=launch)
        want = [KR.sklearn_labels(x, k, theirs)[0] for x, k in ((a, 3), (deg, 5), (b, 6))]
    assert info["fallback"] == [1] and launch.calls == 1
    assert all(np.array_equal(g, w) for g, w in zip(labels, want))
    assert np.array_equal(ours.get_state()[1], theirs.get_state()[1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got, one = kmeans_gpu.k_means_rows(deg, 5, 0, return_info=True, launch=KR.NumpyLaunch())
    assert one["fallback"] is True and np.array_equal(got, KR.sklearn_labels(deg, 5, 0)[0])


def test_wide_inputs_take_the_host_route_and_bad_ones_raise():
    class NoLaunch:
        def __call__(self, *a):
            raise AssertionError("the launch was reached")
    X = KR.blob(200, 33, 3, 3.0, 0)
    got, info = kmeans_gpu.k_means_rows(X, 3, 1, return_info=True, launch=NoLaunch())
    assert info["fallback"] is True and np.array_equal(got, KR.sklearn_labels(X, 3, 1)[0])
    X = KR.blob(300, 4, 33, 4.0, 1)
    labels, info = kmeans_gpu.k_means_groups(np.concatenate([X, X]), [300, 300], [33, 4], [2, 2], return_info=True, launch=KR.NumpyLaunch())
    assert info["fallback"] == [0] and np.array_equal(labels[0], KR.sklearn_labels(X, 33, 2)[0])
    assert np.array_equal(labels[1], KR.sklearn_labels(X, 4, 2)[0])
    bad = KR.blob(50, 2, 2, 2.0, 0)
    bad[7, 1] = np.nan
    with pytest.raises(ValueError, match=r"contains NaN or infinity \(recording\(s\) \[0\]\)"):
        kmeans_gpu.k_means_rows(bad, 2, 0, launch=KR.NumpyLaunch())
    good = KR.blob(50, 2, 2, 2.0, 0)
    for kw, text in ((dict(k=1), "k=1 must lie in"), (dict(k=50), "k=50 must lie in"), (dict(n_init=0), "n_init=0"), (dict(n_init=17), "n_init=17"),
                     (dict(max_iter=0), "max_iter=0"), (dict(tol=-1.0), "tol=-1.0")):
        args = dict(k=2, n_init=10, max_iter=300, tol=1e-4)
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            kmeans_gpu.k_means_rows(good, args.pop("k"), 0, launch=NoLaunch(), **args)
    with pytest.raises(ValueError, match="sizes add up to 49"):
        kmeans_gpu.k_means_groups(good, [20, 29], 2, 0, launch=NoLaunch())
    with pytest.raises(ValueError, match="ks has 3 entries for 2 recordings"):
        kmeans_gpu.k_means_groups(good, [20, 30], [2, 2, 2], 0, launch=NoLaunch())
    # a flag the driver cannot act on names the recording
    with pytest.raises(RuntimeError, match=r"refused recording\(s\) \[0\]"):
        kmeans_gpu.k_means_rows(good, 2, 0, launch=lambda X, fr, ks, *rest: (np.full(50, -1, np.int32), np.array([-1]), np.zeros(1), np.zeros(1, int),
                                                                            np.array([KR.BAD_PROMISE])))


def test_there_is_no_cpu_fallback():
    X = KR.blob(50, 2, 2, 2.0, 0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="the device k-means route takes the rows as a GPU tensor; there is no CPU fallback"):
            kmeans_gpu.k_means_rows(X, 2, 0)
    with pytest.raises(RuntimeError, match="there is no CPU fallback"):
        kmeans_gpu.k_means_rows(torch.from_numpy(X), 2, 0)
    z = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kmeans_grouped(torch.from_numpy(X), z[:2], z[:1], z[:1].reshape(1, 1), torch.zeros((1, 1, 31, 5), dtype=torch.float64), 1, 300, 1e-4)
    assert "launch(X, first_row, ks, first, u, n_init, max_iter, tol)" in kmeans_gpu.__doc__


# ------------------------------------------------------------------ the public routes

@pytest.mark.parametrize("n,k,noise,seed", [(400, 2, 0.9, 0), (700, 3, 1.5, 0), (1000, 4, 2.0, 0), (2000, 8, 1.2, 0)])
def test_spectral_with_device_labels_equals_the_sklearn_route_on_the_cpu(n, k, noise, seed):
    X, _ = R.planted_rows(n, k, noise, seed)
    K = R.cosine(X).astype(np.float32)
    want = cluster_gpu.spectral(None, k, operator=R.NumpyOperator(K))
    launch = KR.NumpyLaunch()
    got, info = cluster_gpu.spectral(None, k, operator=R.NumpyOperator(K), assign_labels="device", kmeans_launch=launch, return_info=True)
    assert all(v >= KR.MARGIN_BAR for v in launch.trace.margins.values()), launch.trace.margins
    assert launch.calls == 1 and np.array_equal(got, want) and got.dtype == want.dtype
    assert info["kmeans"]["fallback"] is False and 0 <= info["kmeans"]["chosen"] < 10


def test_the_routes_are_opt_in():
    assert inspect.signature(cluster_gpu.spectral).parameters["assign_labels"].default == "sklearn"
    assert inspect.signature(cluster_gpu.spectral_embedding).parameters["on_device"].default is False
    with pytest.raises(ValueError, match="assign_labels='gpu'"):
        cluster_gpu.spectral(None, 2, operator=R.NumpyOperator(np.eye(4, dtype=np.float32)), assign_labels="gpu")
    # the early returns do not reach the k-means
    for n, ks in ((0, 2), (3, 1), (3, 3), (3, 5)):
        K = np.ones((n, n), np.float32)
        assert np.array_equal(cluster_gpu.spectral(None, ks, operator=R.NumpyOperator(K), assign_labels="device"),
                              cluster_gpu.spectral(None, ks, operator=R.NumpyOperator(K)))
    assert inspect.signature(db.diarize_audio).parameters["clustering"].default == "spectral"
    assert inspect.signature(db.Diarizer.__init__).parameters["clustering"].default == "spectral"
    assert inspect.signature(db.diarize_audios).parameters["clustering"].default == "ahc_gpu"
    assert db.Diarizer(db.DiarizationParameters(), clustering="spectral_device").clustering == "spectral_device"
    tool = open(os.path.join(os.path.dirname(HERE), "tools", "diarize_sharded.py")).read()
    assert re.search(r'choices=\("spectral", "ahc", "spectral_gpu", "spectral_device", "ahc_gpu"\)', tool)
    audio = {"waveform": np.zeros(16000, np.float32), "sample_rate": 16000}
    with pytest.raises(ValueError, match="speaker_bounds=True bounds the cluster count of clustering='ahc_gpu'"):
        db.diarize_audio(audio, 0.35, 0.1, 2, 6, clustering="spectral_device", speaker_bounds=True, encoder=lambda w: None)
    with pytest.raises(ValueError, match="speaker_bounds=True"):
        db.Diarizer(db.DiarizationParameters(), clustering="spectral_device", speaker_bounds=True)
    with pytest.raises(ValueError, match="ahc_gpu"):
        db.diarize_audios([audio], 0.35, 0.1, 2, 6, clustering="spectral_device")


def test_pipeline_refuses_spectral_device_with_an_injected_encoder():
    from speech_diarization_amd import synth
    y = synth.synthetic_conversation(12.0, 2, seed=0).wav

    def enc(w):
        return np.stack([np.abs(np.fft.rfft(r, 382))[:192] for r in np.asarray(w, dtype=np.float32)]).astype(np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        db.diarize_audio({"waveform": y, "sample_rate": 16000}, 0.35, 0.1, 2, 6, encoder=enc, clustering="spectral_device")
