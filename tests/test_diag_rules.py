"""No-GPU checks of the f64 whitening / centroid entries (include/sd_hip_diag.h, speech-diarization_amd/csrc/diag/): the census rule
of tests/test_launch_log_rules.py for the new source directory (every kernel has a launch label, every label a GPU test of
tests/test_gpu_diag.py that asserts it ran), the binding table, the versions, the workspace formula and the refusals an entry makes
before it launches anything."""
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import launch_log as L  # noqa: E402
from abi_rules import ARG, UNSUP, WS, check_header_and_table, check_versions, refused  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402

DIAG = N.PKG_DIR / "csrc" / "diag"
LABEL = re.compile(r'SD_CHECK_LAUNCH\("([a-z0-9_]+_kernel)"\)')

# label -> the function of tests/test_gpu_diag.py that runs it under expect_launches
KERNEL_TESTS = {
    "whiten_colsum_kernel": "test_stats_are_exact_on_integer_rows",
    "whiten_mean_kernel": "test_stats_are_exact_on_integer_rows",
    "whiten_gram_kernel": "test_stats_are_exact_on_integer_rows",
    "whiten_gram_finish_kernel": "test_stats_are_exact_on_integer_rows",
    "whiten_apply_kernel": "test_apply_is_exact_on_signed_permutations",
    "label_centroids_kernel": "test_centroids_are_exact_on_integer_rows",
}


def _sources():
    return {f.name: f.read_text() for f in sorted(DIAG.glob("*.hip"))}


def _function_text(text, fn):
    m = re.search(rf"^def {fn}\(.*?(?=^\S)", text + "\nend", flags=re.M | re.S)
    return m.group(0) if m else None


# ------------------------------------------------------------------ the census of the directory

def test_every_kernel_of_the_directory_has_a_label():
    text = "".join(_sources().values())
    kernels = set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", text))
    assert len(kernels) == 6 and all(k.endswith("_kernel") for k in kernels), sorted(kernels)
    labels = set(LABEL.findall(text))
    assert kernels == labels == set(KERNEL_TESTS), (sorted(kernels ^ labels), sorted(labels ^ set(KERNEL_TESTS)))
    assert len(re.findall(r"\bSD_CHECK_LAUNCH\(", text)) == len(labels)        # one launch site each, each with a literal
    assert len(re.findall(r"\bhipLaunchKernelGGL\(", text)) == len(labels)
    # the directory's labels do not collide with the census of csrc/*.hip, which stays as it is
    import kernel_census
    assert not labels & {L.kernel_of(lb) for lb in kernel_census.KERNEL_TESTS}


def test_every_label_is_asserted_by_a_gpu_test():
    text = open(os.path.join(HERE, "test_gpu_diag.py")).read()
    assert "pytestmark = pytest.mark.gpu" in text
    for label, fn in KERNEL_TESTS.items():
        body = _function_text(text, fn)
        assert body, (label, fn)
        assert "expect_launches" in body and label in body, (label, fn)
    # the rule bites: a test that never names the kernel is not accepted for it
    body = _function_text(text, "test_centroids_are_exact_on_integer_rows")
    assert "whiten_apply_kernel" not in body


def test_no_floating_point_atomics_and_the_f64_matrix_core():
    text = "".join(_sources().values())
    code = re.sub(r"//.*", "", text)
    assert "atomic" not in code
    assert code.count("__builtin_amdgcn_mfma_f64_16x16x4f64") == 2            # the Gram tile and the transform


# ------------------------------------------------------------------ ABI

def test_header_and_binding_table_name_the_same_exported_entries():
    names = check_header_and_table("sd_hip_diag.h", N.DIAG_PROTOTYPES,
                                   (N.PROTOTYPES, N.SPECTRAL_PROTOTYPES, N.AHC_PROTOTYPES, N.HDBSCAN_PROTOTYPES, N.TRACE_PROTOTYPES))
    assert names == {"sd_diag_abi_version", "sd_whiten_stats_workspace_bytes", "sd_whiten_stats_f64", "sd_whiten_apply_f64", "sd_label_centroids_f32"}
    main = open(N.PKG_DIR.parent / "include" / "sd_hip.h").read()
    assert not any(n in main for n in names)                         # nothing was added to the main header


def test_versions_and_struct_sizes():
    lib = N.load()
    assert N.SD_DIAG_ABI_VERSION == 1
    check_versions(sd_diag_abi_version=1, sd_trace_abi_version=3, sd_abi_version=11, sd_spectral_abi_version=1, sd_ahc_abi_version=1,
                   sd_hdbscan_abi_version=1)
    assert [int(lib.sd_sizeof(i)) for i in range(5)] == [184, 88, 1672, 13944, 0]


def test_workspace_formula():
    """B row blocks of 512 rows; per block 16 T column sums and one 16 x 16 tile for each of the T (T + 1) / 2 tile pairs."""
    lib = N.load()
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_diag.h").read()
    assert re.search(r"#define\s+SD_WHITEN_ROWS\s+512\b", header)
    for n in (2, 40, 511, 512, 513, 1030, 50000):
        b = -(-n // 512)
        for d in (1, 4, 16, 17, 20, 190, 192, 200, 256):
            t = -(-d // 16)
            assert int(lib.sd_whiten_stats_workspace_bytes(n, d)) == b * (16 * t + 256 * t * (t + 1) // 2) * 8, (n, d)
    assert int(lib.sd_whiten_stats_workspace_bytes(2000, 192)) == 4 * (192 + 256 * 78) * 8
    for n, d in ((1, 192), (0, 192), (-3, 192), (100, 0), (100, -1), (100, 257)):
        assert int(lib.sd_whiten_stats_workspace_bytes(n, d)) == 0, (n, d)


# ------------------------------------------------------------------ refusals before launch (no device needed: fake non-null pointers)

def _stats(lib, x=0x1000, ld=192, n=100, d=192, mean=0x2000, gram=0x3000, ldg=None, ws=0x5000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = int(lib.sd_whiten_stats_workspace_bytes(n, d))
    return lib.sd_whiten_stats_f64(x, ld, n, d, mean, gram, d if ldg is None else ldg, ws, ws_bytes, None)


def _apply(lib, x=0x1000, ld=192, n=100, d=192, mean=0x2000, w=0x3000, ldw=None, eps=1e-9, out=0x4000, ldo=None):
    return lib.sd_whiten_apply_f64(x, ld, n, d, mean, w, d if ldw is None else ldw, eps, out, d if ldo is None else ldo, None)


def _centroids(lib, x=0x1000, ld=192, n=100, d=192, labels=0x2000, k=4, eps=1e-9, out=0x3000, ldo=None, count=0x4000):
    return lib.sd_label_centroids_f32(x, ld, n, d, labels, k, eps, out, d if ldo is None else ldo, count, None)


def test_refusals_happen_before_anything_is_launched():
    """Every case returns its own argument / support / workspace code and sets sd_last_error.  A launch on this pointer soup would
    have returned SD_ERR_HIP (no device here) or faulted (on a GPU)."""
    lib = N.load()
    for name in ("x", "mean", "gram", "ws"):
        refused(_stats(lib, **{name: None}), ARG, "null pointer")
    for name in ("x", "mean", "w", "out"):
        refused(_apply(lib, **{name: None}), ARG, "null pointer")
    for name in ("x", "labels", "out", "count"):
        refused(_centroids(lib, **{name: None}), ARG, "null pointer")
    for call, who in ((_stats, "sd_whiten_stats_f64"), (_apply, "sd_whiten_apply_f64"), (_centroids, "sd_label_centroids_f32")):
        refused(call(lib, n=0), ARG, "n=0")
        refused(call(lib, n=-5), ARG, "n=-5")
        refused(call(lib, d=0), ARG, "d=0")
        refused(call(lib, d=192, ld=188), ARG, "ld=188")
        refused(call(lib, d=257, ld=260), UNSUP, "d=257")
        refused(call(lib, x=0x1004), ARG, "16-byte aligned")
        refused(call(lib, x=0x1008), ARG, "16-byte aligned")
        refused(call(lib, d=190, ld=190), ARG, "ld=190")
        refused(call(lib, d=7, ld=9), ARG, "ld=9")
        assert who in N.last_error()
    refused(_stats(lib, n=1), ARG, "n=1")                             # one row has no covariance
    refused(_stats(lib, ldg=191), ARG, "ldg=191")
    refused(_stats(lib, ws=0x5008), ARG, "aligned")
    need = int(lib.sd_whiten_stats_workspace_bytes(100, 192))
    refused(_stats(lib, ws_bytes=need - 1), WS, "workspace")
    refused(_stats(lib, ws_bytes=0), WS, "workspace")
    refused(_apply(lib, ldw=191), ARG, "ldw=191")
    refused(_apply(lib, ldo=100), ARG, "ldo=100")
    refused(_centroids(lib, k=0), ARG, "k=0")
    refused(_centroids(lib, k=1025), UNSUP, "k=1025")
    refused(_centroids(lib, ldo=191), ARG, "ldo=191")


def test_build_list_and_fingerprint_cover_the_directory():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sd_build_native_diag", str(N.PKG_DIR / "build_native.py"))
    bn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bn)
    assert "diag/sd_diag.hip" in bn.SOURCES and all((bn.CSRC / s).exists() for s in bn.SOURCES)
    assert len({os.path.basename(s) for s in bn.SOURCES}) == len(bn.SOURCES)             # object files are named by the stem
    src = (N.PKG_DIR / "build_native.py").read_text()
    assert '(CSRC / "diag").glob' in _function_text(src, "_fingerprint")
