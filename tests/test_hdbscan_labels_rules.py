"""No-GPU checks of the device labelling of HDBSCAN (include/sd_hip_tree.h: sd_tree_labels_grouped, speech-diarization_amd/csrc/tree/,
`hdbscan_gpu.hdbscan_rows(..., labelling="device")`): the header and its binding table, the untouched versions, the census of the new
source directory, the pure check (csrc/tree/sd_tree_check.h, built alone with sanitizers) with its codes and precedence, the workspace
formula on both sides of the LDS cap, the numpy restatement of the algorithm against the scikit-learn oracle on every case of the GPU
test, and the drivers run on the CPU through a numpy operator that has `tree_labels`."""
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
import hdbscan_grouped_ref as HG  # noqa: E402
import hdbscan_labels_ref as T  # noqa: E402
import hdbscan_ref as H  # noqa: E402
import launch_log as L  # noqa: E402
from abi_rules import ARG, UNSUP, WS, check_header_and_table, check_versions, refused  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import cluster, hdbscan_gpu, ops  # noqa: E402

TREE = N.PKG_DIR / "csrc" / "tree"
CSRC = N.PKG_DIR / "csrc"
NAMES = {"sd_tree_abi_version", "sd_tree_labels_workspace_bytes", "sd_tree_labels_grouped"}
ENTRY = "sd_tree_labels_grouped"


# ------------------------------------------------------------------ ABI

def test_header_and_binding_table_name_the_same_exported_entries():
    others = (N.PROTOTYPES, N.SPECTRAL_PROTOTYPES, N.AHC_PROTOTYPES, N.HDBSCAN_PROTOTYPES, N.DIAG_PROTOTYPES, N.TRACE_PROTOTYPES)
    assert check_header_and_table("sd_hip_tree.h", N.TREE_ENTRIES, others) == NAMES
    # through the table they reach `ops.launch` by themselves; the six *_PROTOTYPES tables and their union stay what they were
    assert NAMES <= ops._LAUNCHABLE and ops._LAUNCHABLE == ops._ENTRIES | NAMES and not NAMES & ops._ENTRIES
    assert '("sd_hip_tree.h", TREE_ENTRIES, "sd_tree_abi_version", SD_TREE_ABI_VERSION, "tree ")' in open(N.__file__).read()


def test_the_new_version_is_one_and_every_other_is_untouched():
    assert N.SD_TREE_ABI_VERSION == 1
    check_versions(sd_tree_abi_version=1, sd_abi_version=11, sd_spectral_abi_version=1, sd_ahc_abi_version=1, sd_hdbscan_abi_version=1,
                   sd_diag_abi_version=1, sd_trace_abi_version=3)
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_tree.h").read()
    assert re.search(r"#define\s+SD_TREE_ABI_VERSION\s+1\b", header)


# ------------------------------------------------------------------ the census of the directory

def test_the_directory_has_one_kernel_with_one_labelled_launch():
    srcs = {f.name: f.read_text() for f in sorted(TREE.glob("*"))}
    assert sorted(srcs) == ["sd_tree_check.h", "sd_tree_labels.hip"]
    text = srcs["sd_tree_labels.hip"]
    kernels = set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", text))
    assert kernels == {"tree_labels_grouped_kernel"}
    assert re.findall(r'\bSD_CHECK_LAUNCH\("([a-z0-9_]+)"\)', text) == ["tree_labels_grouped_kernel"]
    assert len(re.findall(r"\bhipLaunchKernelGGL\(", text)) == 1
    code = re.sub(r"//.*", "", text)
    assert "atomic" not in code and "fast-math" not in code and "#pragma clang fp contract(off)" in code
    # the entry refuses through the one pure check and has no argument check of its own
    assert not re.search(r"\bSD_CHECK_ARG\(", code) and len(re.findall(r"\bsd_tree_check\(", code)) == 1
    assert len(re.findall(r"\bsd_set_error\(", code)) == 1 and len(re.findall(r"\bsd_tree_workspace_bytes\(", code)) == 1
    # outside the census of csrc/*.hip and of the other directories
    import kernel_census
    assert not kernels & {L.kernel_of(lb) for lb in kernel_census.KERNEL_TESTS}
    for other in ("ahc", "diag", "hdbscan"):
        theirs = "".join(f.read_text() for f in sorted((CSRC / other).glob("*")))
        assert not kernels & set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", theirs))
    # the check is pure: no HIP, nothing but the status codes
    raw = srcs["sd_tree_check.h"]
    assert re.findall(r'#include [<"]([^>"]+)[>"]', raw) == ["limits.h", "stdio.h", "sd_hip.h"] and "hip" not in re.sub(r"//.*|sd_hip\.h", "", raw).lower()


def test_the_label_is_asserted_by_the_gpu_tests():
    text = open(os.path.join(HERE, "test_gpu_hdbscan_labels.py")).read()
    assert "pytestmark = pytest.mark.gpu" in text
    assert re.search(r'KERNEL = "tree_labels_grouped_kernel"', text)
    tests = re.findall(r"^def (test_\w+)\(.*?(?=^def |\Z)", text, flags=re.M | re.S)
    bodies = re.findall(r"^def test_\w+\(.*?(?=^def |\Z)", text, flags=re.M | re.S)
    assert len(tests) >= 5 and all("expect_launches" in b or "_launch(" in b or "_run(" in b for b in bodies), tests
    assert "expect_launches(exactly={KERNEL})" in text


def test_build_list_and_fingerprint_cover_the_directory():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sd_build_native_tree", str(N.PKG_DIR / "build_native.py"))
    bn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bn)
    assert "tree/sd_tree_labels.hip" in bn.SOURCES and all((bn.CSRC / s).exists() for s in bn.SOURCES)
    assert len({os.path.basename(s) for s in bn.SOURCES}) == len(bn.SOURCES)
    assert '(CSRC / "tree").glob' in (N.PKG_DIR / "build_native.py").read_text()
    assert not any("fast" in f for f in bn.compile_flags())            # the stabilities need IEEE division and separate roundings


# ------------------------------------------------------------------ the pure check

@pytest.fixture(scope="module")
def pure(tmp_path_factory):
    cxx = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(cxx), "no clang++ on this machine"
    exe = tmp_path_factory.mktemp("tree_check") / "tree_check_pure"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           f"-I{N.PKG_DIR.parent / 'include'}", os.path.join(HERE, "helpers", "tree_check_pure.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(*calls):
        ran = subprocess.run([str(exe), *calls], capture_output=True, text=True)
        assert ran.returncode == 0 and not ran.stderr, (ran.returncode, ran.stderr[-2000:])
        return ran.stdout.splitlines()
    return run


CAP = T.LDS_ROWS
I31 = 2 ** 31 - 1
# (n_edges, n_groups, max_edges, min_cluster_size, allow_single_cluster, ws_bytes (-1: the need), flags) -> (status, text in the message)
REFUSALS = [
    ((100, 0, 10, 2, 1, -1, "-"), ARG, "n_edges=100 n_groups=0"),
    ((100, -1, 10, 2, 1, -1, "-"), ARG, "n_groups=-1"),
    ((2, 3, 10, 2, 1, -1, "-"), ARG, "n_edges=2 n_groups=3 (every recording has at least one edge)"),
    ((100, 3, 0, 2, 1, -1, "-"), ARG, "max_edges=0"),
    ((100, 3, -4, 2, 1, -1, "-"), ARG, "max_edges=-4"),
    ((I31, 1, 10, 2, 1, -1, "-"), UNSUP, f"at most {I31} rows are supported"),
    ((I31 - 1, 1, I31, 2, 1, -1, "-"), UNSUP, f"a recording of at most {2 ** 30} rows is supported"),
    ((100, 3, 50, 1, 1, -1, "-"), ARG, "min_cluster_size=1 must be at least 2"),
    ((100, 3, 50, 2, 2, -1, "-"), ARG, "allow_single_cluster=2 must be 0 or 1"),
    ((100, 3, 50, 2, -1, -1, "-"), ARG, "allow_single_cluster=-1"),
    ((100, 3, 50, 2, 1, -1, "p"), ARG, "null pointer"),
    ((100, 3, 50, 2, 1, -1, "d"), ARG, "dist must be 8-byte aligned"),
    ((9000, 3, CAP, 2, 1, -1, "w"), ARG, "null pointer"),
    ((9000, 3, CAP, 2, 1, -1, "m"), ARG, "workspace is not 16-byte aligned"),
    ((9000, 3, CAP, 2, 1, 72 * 9003 - 1, "-"), WS, f"workspace of {72 * 9003 - 1} bytes, n_edges=9000 n_groups=3 max_edges={CAP} needs {72 * 9003}"),
    ((9000, 3, CAP, 2, 1, 0, "-"), WS, "workspace of 0 bytes"),
    # precedence: the shape, max_edges, the two size limits, min_cluster_size, allow_single_cluster, the pointers, dist, the workspace
    ((2, 3, 0, 1, 2, 0, "pdwm"), ARG, "n_edges=2 n_groups=3"),
    ((100, 3, 0, 1, 2, 0, "pdwm"), ARG, "max_edges=0"),
    ((I31, 3, I31, 1, 2, 0, "pdwm"), UNSUP, "rows are supported"),
    ((I31 - 9, 3, I31, 1, 2, 0, "pdwm"), UNSUP, "a recording of at most"),
    ((9000, 3, CAP, 1, 2, 0, "pdwm"), ARG, "min_cluster_size=1"),
    ((9000, 3, CAP, 2, 2, 0, "pdwm"), ARG, "allow_single_cluster=2"),
    ((9000, 3, CAP, 2, 0, 0, "pdm"), ARG, "null pointer"),
    ((9000, 3, CAP, 2, 0, 0, "dwm"), ARG, "null pointer"),
    ((9000, 3, CAP, 2, 0, 0, "dm"), ARG, "dist must be"),
    ((9000, 3, CAP, 2, 0, 0, "m"), ARG, "workspace is not"),
]
ACCEPTED = [
    ((1, 1, 1, 2, 0, -1, "-"), 0, 2),
    ((100, 3, 50, 2, 1, -1, "wm"), 0, 51),                              # no bytes needed: the workspace is not looked at
    ((100, 3, 50, 2, 1, 0, "w"), 0, 51),
    ((9000, 3, CAP - 1, 15, 1, -1, "wm"), 0, CAP),
    ((9000, 3, CAP, 15, 1, -1, "-"), 72 * 9003, CAP),
    ((9000, 3, I31, 15, 1, -1, "-"), 72 * 9003, CAP),                   # a bound above n_edges is legal
]


def _call(args):
    return ":".join(str(a) for a in args)


def test_the_pure_check_refuses_with_code_text_and_precedence(pure):
    out = pure(*[_call(args) for args, _, _ in REFUSALS])
    for (args, code, text), line in zip(REFUSALS, out):
        m = re.fullmatch(r"status=(-?\d+) why=(.*)", line)
        assert m and int(m.group(1)) == code and text in m.group(2) and m.group(2).startswith(ENTRY + ": "), (args, line)
    out = pure(*[_call(args) for args, _, _ in ACCEPTED])
    for (args, need, rows), line in zip(ACCEPTED, out):
        assert line == f"status=0 need={need} lds_rows={rows}", (args, line)


def _entry(lib, n_edges, n_groups, max_edges, mcs, single, ws_bytes, flags):
    """The same description through the built library: fake non-null pointers, nothing can be launched before the check has passed."""
    if ws_bytes < 0:
        ws_bytes = int(lib.sd_tree_labels_workspace_bytes(n_edges, n_groups, max_edges))
    p = None if "p" in flags else 0x1000
    return lib.sd_tree_labels_grouped(p, 0x2000, 0x3004 if "d" in flags else 0x3000, 0x4000, n_groups, n_edges, max_edges, mcs, single, 0x5000, 0x6000,
                                      None if "w" in flags else 0x7004 if "m" in flags else 0x7000, ws_bytes, None)


def test_the_entry_is_wired_to_the_check():
    """Every refusal comes back from the entry with the same code and text, before anything is launched (a launch on this pointer soup
    would have returned SD_ERR_HIP here and faulted on a GPU)."""
    lib = N.load()
    for args, code, text in REFUSALS:
        refused(_entry(lib, *args), code, text)
        assert N.last_error().startswith(ENTRY + ": ")
    for name in ("lo", "hi", "dist", "first_edge", "labels", "bad"):
        ptrs = {k: 0x1000 * (i + 1) for i, k in enumerate(("lo", "hi", "dist", "first_edge", "labels", "bad"))}
        ptrs[name] = None
        refused(lib.sd_tree_labels_grouped(ptrs["lo"], ptrs["hi"], ptrs["dist"], ptrs["first_edge"], 3, 100, 50, 2, 1, ptrs["labels"], ptrs["bad"],
                                           None, 0, None), ARG, "null pointer")


def test_workspace_formula_on_both_sides_of_the_cap():
    """72 bytes a row: 8 (sort key) + 8 (stability) + 14 int32.  A CU has 160 KB of LDS, 256 bytes stay with the kernel's static words:
    (163840 - 256) / 72 = 2272 rows, i.e. max_edges <= 2271 needs no workspace and 2272 needs 72 (n_edges + n_groups) bytes."""
    assert T.LDS_ROWS == 2272 == (163840 - 256) // 72 and 72 == 8 + 8 + 14 * 4
    size = N.load().sd_tree_labels_workspace_bytes
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_tree.h").read()
    assert "(160 KB - 256) / 72 = 2272 rows" in header and "72 (n_edges + n_groups)" in header and "for max_edges + 1 <= 2272" in header
    for e, g in ((2271, 1), (5000, 7), (100000, 256), (4544, 2)):
        for m in (1, 500, 2270, 2271):
            assert int(size(e, g, m)) == 0, (e, g, m)
        for m in (2272, 2273, 7608, I31):
            assert int(size(e, g, m)) == 72 * (e + g), (e, g, m)
    assert int(size(2272, 1, 2272)) == 163656 and int(size(121728, 16, 7608)) == 8765568          # 16 recordings of 7 609 rows
    one, two = int(size(100000, 10, 3000)), int(size(200000, 20, 3000))
    assert two == 2 * one                                                                           # linear
    for args in ((0, 1, 5), (5, 0, 5), (5, -1, 5), (2, 3, 5), (5, 1, 0), (5, 1, -2), (I31, 1, 5), (I31 - 1, 1, I31)):
        assert int(size(*args)) == 0, args


# ------------------------------------------------------------------ the restatement against the oracle

def test_the_oracle_is_todays_route_where_no_distances_tie():
    """`oracle_labels` (stable order) equals `_process_mst` + `tree_to_labels`, the calls of `hdbscan_gpu._labels_of_tree`, on distinct
    distances."""
    from sklearn.cluster._hdbscan._tree import tree_to_labels
    from sklearn.cluster._hdbscan.hdbscan import MST_edge_dtype, _process_mst
    for n, seed in ((17, 0), (129, 1), (500, 2)):
        lo, hi, dist = T.random_tree(n, seed, "distinct")
        mst = np.empty(n - 1, dtype=MST_edge_dtype)
        mst["current_node"], mst["next_node"], mst["distance"] = lo, hi, dist
        for mcs, single in T.SETTINGS:
            want = np.asarray(tree_to_labels(_process_mst(mst), mcs, "eom", single, 0.0, None)[0])
            assert np.array_equal(T.oracle_labels(lo, hi, dist, mcs, single), want)


@pytest.mark.parametrize("setting", T.SETTINGS)
def test_small_trees_equal_the_oracle(setting):
    mcs, single = setting
    for name, lo, hi, dist in T.small_trees():
        want = T.oracle_labels(lo, hi, dist, mcs, single)
        assert np.array_equal(T.labels_of_tree_ref(lo, hi, dist, mcs, single), want), name
    if setting == (2, False):                                           # three rows without a single cluster: the root is no candidate
        assert T.oracle_labels(*T.small_trees()[1][1:], mcs, single).tolist() == [-1, -1, -1]
    if setting == (2, True):                                            # the single-root rule: row 1 joins below the largest lambda of the root's entries
        assert T.oracle_labels(*T.small_trees()[1][1:], mcs, single).tolist() == [0, -1, 0]
        assert T.oracle_labels(*T.small_trees()[2][1:], mcs, single).tolist() == [0, 0, 0]


@pytest.mark.parametrize("setting", T.SETTINGS)
def test_the_restatement_equals_the_oracle_on_every_gpu_case(setting):
    """Pins the chain on the CPU: the kernel is held to the oracle, the numpy operator of the driver tests is this restatement."""
    mcs, single = setting
    cases = T.random_cases()
    assert len(cases) == len(T.SIZES) * 9 + 6 and {len(c[3]) + 1 for c in cases} == set(T.SIZES)
    seen = set()
    for name, lo, hi, dist in cases:
        assert T.is_spanning_tree(lo, hi, len(dist) + 1)
        want = T.oracle_labels(lo, hi, dist, mcs, single)
        got = T.labels_of_tree_ref(lo, hi, dist, mcs, single)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, int((got != want).sum()))
        seen.add((int(want.max()) >= 1, bool((want < 0).any())))
    assert any(several for several, _ in seen) and any(noise for _, noise in seen)        # the cases are no trivial ones


def test_the_families_are_what_they_say():
    for n in (17, 500):
        assert len(np.unique(T.random_tree(n, 0, "distinct")[2])) == n - 1
        assert set(np.unique(T.random_tree(n, 0, "four")[2]).tolist()) <= {0.25, 0.5, 0.75, 1.25}
        assert int((T.random_tree(n, 0, "zeros")[2] == 0.0).sum()) == (n - 1) // 4
    lo, hi, dist, first, max_edges = T.pack([T.random_tree(17, 0), T.random_tree(3, 0), T.random_tree(64, 0)])
    assert first.tolist() == [0, 16, 18, 81] and max_edges == 63 and len(lo) == len(hi) == len(dist) == 81
    assert [len(x) for x in T.unpack(np.arange(84), first)] == [17, 3, 64]


def test_the_numpy_entry_reports_broken_recordings():
    trees = [T.random_tree(17, 0), T.random_tree(64, 1, "four"), T.random_tree(129, 2, "zeros")]
    want = [T.labels_of_tree_ref(*t, 2, True) for t in trees]
    for kind in ("cycle", "high", "negative", "nan"):
        broken = T.break_tree(trees[1], kind)
        labels, bad = T.tree_labels_numpy(*T.pack([trees[0], broken, trees[2]])[:4], 128, 2, True)
        per = T.unpack(labels, T.pack(trees)[3])
        assert bad.tolist() == [0, 1, 0] and (per[1] == -1).all() and np.array_equal(per[0], want[0]) and np.array_equal(per[2], want[2]), kind
    labels, bad = T.tree_labels_numpy(*T.pack(trees)[:4], 100, 2, True)
    assert bad.tolist() == [0, 0, 1]


# ------------------------------------------------------------------ the drivers on the CPU

class Recording(T.NumpyLabelRows):
    """Keeps what `tree_labels` was handed."""

    def tree_labels(self, lo, hi, dist, first_edge, *rest):
        self.seen = (lo.numpy().copy(), hi.numpy().copy(), dist.numpy().copy(), first_edge.numpy().copy())
        return super().tree_labels(lo, hi, dist, first_edge, *rest)


# planted(n, k, noise, seed, outliers): at (2, None) the tree's weights are raw scores (core[i] >= every score of row i); the seeds are
# those at which the f32 weights of the numpy operator are pairwise distinct (asserted below, and again on the GPU's own weights)
PLANTED = [(300, 4, 0.6, 0, 0), (500, 5, 0.8, 1, 10), (129, 3, 0.5, 5, 4)]


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_hdbscan_rows_device_equals_sklearn_where_no_distances_tie(metric):
    several = 0
    for shape in PLANTED:
        X = torch.from_numpy(H.planted(*shape))
        op = Recording()
        got, info = hdbscan_gpu.hdbscan_rows(X, 2, None, True, metric, operator=op, labelling="device", return_info=True)
        want, winfo = hdbscan_gpu.hdbscan_rows(X, 2, None, True, metric, operator=op, return_info=True)
        lo, hi, dist, first = op.seen
        assert len(np.unique(dist)) == len(dist) == shape[0] - 1 and first.tolist() == [0, shape[0] - 1], shape
        assert got.dtype == want.dtype and np.array_equal(got, want) and info["mst_weight"] == winfo["mst_weight"], shape
        assert op.label_calls == 1
        several += int(want.max()) >= 1
    assert several >= 1                                                 # not only inputs that end as one cluster


@pytest.mark.parametrize("setting", H.SETTINGS)
def test_hdbscan_rows_device_equals_the_oracle_on_the_same_edges(setting):
    """At min_samples >= 3 the weights tie (the module's docstring): the device labelling is the oracle on the edges the driver built,
    whether or not the unstable argsort of the scikit-learn route agrees."""
    mcs, ms, single = setting
    for shape in PLANTED[:2]:
        op = Recording()
        got = hdbscan_gpu.hdbscan_rows(torch.from_numpy(H.planted(*shape)), mcs, ms, single, operator=op, labelling="device")
        lo, hi, dist, _ = op.seen
        assert np.array_equal(got, T.oracle_labels(lo, hi, dist, mcs, single)), (shape, setting)


@pytest.mark.parametrize("setting", H.SETTINGS)
def test_groups_device_equal_one_call_per_recording(setting):
    """The folder of tests/test_hdbscan_grouped_rules.py (sizes 0, 1, 2, 3, identical rows and the recorded tie input among them): ONE
    `tree_labels` call labels every recording, each as its own call does."""
    mcs, ms, single = setting
    recs = [(name, x) for name, x in HG.driver_recordings() if len(x) < 2 or (ms or mcs) <= len(x)]
    X = np.concatenate([x for _, x in recs])
    op = Recording()
    rows = op.normalise(torch.from_numpy(X))
    op.normalise = lambda _X: rows
    labels, info = hdbscan_gpu.hdbscan_rows_groups(torch.from_numpy(X), [len(x) for _, x in recs], mcs, ms, single, operator=op,
                                                   labelling="device", return_info=True)
    assert op.label_calls == 1 and len(op.seen[3]) - 1 == sum(1 for _, x in recs if len(x) >= 2)
    bounds = np.concatenate([[0], np.cumsum([len(x) for _, x in recs])])
    for i, ((name, x), got) in enumerate(zip(recs, labels)):
        a, b = int(bounds[i]), int(bounds[i + 1])
        lone = op.alone(rows, a, b)
        lone.normalise = lambda _X, a=a, b=b: rows[a:b]
        lone.tree_labels = T.NumpyLabelRows().tree_labels
        want, winfo = hdbscan_gpu.hdbscan_rows(torch.from_numpy(x), mcs, ms, single, operator=lone, labelling="device", return_info=True)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), name
        assert info["mst_weight"][i] == winfo["mst_weight"]


def test_device_labelling_runs_without_scikit_learns_private_modules(monkeypatch):
    for name in ("sklearn.cluster._hdbscan", "sklearn.cluster._hdbscan._tree", "sklearn.cluster._hdbscan.hdbscan",
                 "sklearn.cluster._hdbscan._linkage", "sklearn.cluster._hdbscan._reachability"):
        monkeypatch.setitem(sys.modules, name, None)
    X = torch.from_numpy(H.planted(*PLANTED[2]))
    with pytest.raises(ImportError, match="private functions of scikit-learn 1.7.2"):
        hdbscan_gpu.hdbscan_rows(X, operator=T.NumpyLabelRows())
    with pytest.raises(ImportError, match="private functions"):
        hdbscan_gpu.hdbscan_rows_groups(X, [100, 29], operator=T.NumpyLabelRows())
    one = hdbscan_gpu.hdbscan_rows(X, operator=T.NumpyLabelRows(), labelling="device")
    many = hdbscan_gpu.hdbscan_rows_groups(X, [100, 0, 29], operator=T.NumpyLabelRows(), labelling="device")
    assert one.shape == (129,) and [len(m) for m in many] == [100, 0, 29] and int(one.max()) >= 1
    src = open(hdbscan_gpu.__file__).read()
    assert len(re.findall(r"^\s*from sklearn|^\s*import sklearn", src, flags=re.M)) == 2              # both inside _sklearn_tree()


def test_tiny_refused_and_bad_inputs():
    class NoLabels(T.NumpyLabelRows):
        def tree_labels(self, *a):
            raise AssertionError("tree_labels reached")
    rows, groups = hdbscan_gpu.hdbscan_rows, hdbscan_gpu.hdbscan_rows_groups
    assert rows(torch.zeros(1, 4), operator=NoLabels(), labelling="device").tolist() == [0]
    assert rows(torch.zeros(0, 4), operator=NoLabels(), labelling="device").tolist() == []
    assert [g.tolist() for g in groups(torch.zeros(3, 4), [1, 0, 1, 1], operator=NoLabels(), labelling="device")] == [[0], [], [0], [0]]
    X = torch.from_numpy(H.planted(*PLANTED[0]))
    for fn, args in ((rows, ()), (groups, ([100, 200],))):
        with pytest.raises(ValueError, match=r"labelling must be one of \('sklearn', 'device'\), got 'gpu'"):
            fn(X, *args, operator=T.NumpyLabelRows(), labelling="gpu")
        with pytest.raises(TypeError, match="needs an operator with tree_labels"):
            fn(X, *args, operator=HG.NumpyGroupedRows(), labelling="device")
    two = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0]], np.float32)
    got = groups(torch.from_numpy(np.concatenate([two[:1], two, two[1:]])), [1, 2, 1], operator=T.NumpyLabelRows(), labelling="device")
    assert [g.tolist() for g in got] == [[0], [0, 0], [0]]

    class Breaks(T.NumpyLabelRows):                                     # an operator that hands the entry a cycle in its second tree
        def tree_labels(self, lo, hi, dist, first_edge, *rest):
            lo, hi = lo.clone(), hi.clone()
            a = int(first_edge[1])
            lo[a + 1], hi[a + 1] = lo[a], hi[a]
            return super().tree_labels(lo, hi, dist, first_edge, *rest)
    with pytest.raises(RuntimeError, match=r"recording 2: its 199 edges are not a spanning tree of its 200 rows"):
        groups(X, [100, 0, 200], operator=Breaks(), labelling="device")


def test_no_cpu_fallback_and_the_public_names():
    from speech_diarization_amd import anti_stick_diarize as asd
    lo = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tree_labels_grouped(lo, lo, torch.zeros(3, dtype=torch.float64), torch.tensor([0, 3], dtype=torch.int32), 3, 2, True)
    X = H.planted(*PLANTED[2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hdbscan_gpu.hdbscan_rows(torch.from_numpy(X), labelling="device")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            asd.cluster_hdbscan(X, use_gpu="rows_device")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            hdbscan_gpu.HdbscanGpuClusterer(labelling="device").fit_predict(X)
    with pytest.raises(ValueError, match="use_gpu must be False, True or 'rows'"):
        asd.cluster_hdbscan(X, use_gpu="device")
    with pytest.raises(ValueError, match="takes no clusterer_factory"):
        asd.cluster_hdbscan(X, use_gpu="rows_device", clusterer_factory=cluster.default_hdbscan_factory)
    with pytest.raises(ValueError, match="labelling must be one of"):
        hdbscan_gpu.HdbscanGpuClusterer(labelling="host")
    made = hdbscan_gpu.HdbscanGpuClusterer.factory(labelling="device")(min_cluster_size=5, metric="cosine")
    assert made.labelling == "device" and made.min_cluster_size == 5 and made.metric == "cosine"
    assert hdbscan_gpu.HdbscanGpuClusterer.factory()(min_cluster_size=2).labelling == "sklearn" == hdbscan_gpu.HdbscanGpuClusterer().labelling
    import inspect
    for fn in (hdbscan_gpu.hdbscan_rows, hdbscan_gpu.hdbscan_rows_groups, hdbscan_gpu.HdbscanGpuClusterer.__init__, hdbscan_gpu.HdbscanGpuClusterer.factory):
        assert inspect.signature(fn).parameters["labelling"].default == "sklearn", fn
    for other in ("hdbscan_two_stage", "ahc", "hdbscan_labels"):
        with pytest.raises(ValueError, match="hdbscan_gpu"):
            asd.diarize_many([np.zeros(16000, np.float32)], clusterer=other)
    assert "tree_labels(lo, hi, dist, first_edge, max_edges, min_cluster_size, allow_single_cluster)" in hdbscan_gpu.__doc__


def test_two_stage_through_the_device_factory_equals_the_sklearn_factory():
    X = H.planted(*PLANTED[2])                                          # several micro-clusters: stage 2 runs
    ops_seen = []

    def factory(labelling):
        def make(**kw):
            ops_seen.append(Recording())
            return hdbscan_gpu.HdbscanGpuClusterer(kw["min_cluster_size"], kw["min_samples"], kw["allow_single_cluster"], kw["metric"],
                                                   operator=ops_seen[-1], labelling=labelling)
        return make
    got = cluster.cluster_hdbscan_two_stage(X, 2, clusterer_factory=factory("device"))
    assert len(ops_seen) == 2 and all(op.label_calls == 1 for op in ops_seen)                          # both stages
    assert all(len(np.unique(op.seen[2])) == len(op.seen[2]) for op in ops_seen)                       # no ties: the two labellings agree
    want = cluster.cluster_hdbscan_two_stage(X, 2, clusterer_factory=factory("sklearn"))
    assert got.dtype == want.dtype and np.array_equal(got, want) and len(set(got.tolist())) >= 2


def _fft_encoder(w):
    return np.stack([np.abs(np.fft.rfft(r, 382))[:192] for r in np.asarray(w, dtype=np.float32)]).astype(np.float32)


def _vad(y, sr, **kw):
    if not np.any(y):
        return []
    return [(0.5 * i, 0.5 * i + 0.45) for i in range(int(len(y) / sr / 0.5))]


def test_diarize_and_diarize_many_take_the_device_clusterer(monkeypatch):
    """Stub encoder and stub VAD; the product factory is patched to the numpy operator and records the labelling it was asked for."""
    from speech_diarization_amd import anti_stick_diarize as asd
    from speech_diarization_amd import synth
    ys = [synth.synthetic_conversation(20.0, 2, seed=0).wav, np.zeros(3 * 16000, np.float32), synth.synthetic_conversation(12.0, 3, seed=1).wav]
    kw = dict(encode=_fft_encoder, vad_segments=_vad, scd_thr=1e9, reseg=0)
    product_factory = hdbscan_gpu.HdbscanGpuClusterer.factory
    asked = []

    def factory(operator=None, labelling="sklearn"):
        assert operator is None
        asked.append(labelling)
        return product_factory(operator=T.NumpyLabelRows(), labelling=labelling)
    monkeypatch.setattr(hdbscan_gpu.HdbscanGpuClusterer, "factory", staticmethod(factory))
    triples = lambda segs: [(s.start, s.end, s.spk) for s in segs]  # noqa: E731
    want = [asd.diarize(y, **kw, clusterer="hdbscan_device") for y in ys]
    assert asked == ["device"] * 2                                     # the silent recording never reaches the clusterer
    asked.clear()
    got = asd.diarize_many(ys, **kw, clusterer="hdbscan_device")
    assert asked == ["device"] and [triples(g) for g in got] == [triples(w) for w in want] and got[1] == [] and len(got[0]) >= 1
    asked.clear()
    asd.diarize_many(ys, **kw)
    asd.diarize(ys[0], **kw, clusterer="hdbscan_gpu")
    assert asked == ["sklearn", "sklearn"]                             # the defaults are what they were
