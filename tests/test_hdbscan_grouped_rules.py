"""No-GPU checks of the grouped HDBSCAN route (include/sd_hip_hdbscan.h: sd_hdb_core_grouped_f32 and sd_hdb_outgoing_grouped_f32,
speech-diarization_amd/csrc/hdbscan/, `hdbscan_gpu.hdbscan_rows_groups`): the census rule of tests/test_launch_log_rules.py for the new
source directory, the binding table, the untouched versions, the two workspace formulas and their linear growth, the refusals the
entries make before they launch anything, the driver itself run on the CPU through a numpy operator with the group mask against
`hdbscan_rows` on every recording alone, the two-stage glue for many recordings, and `diarize_many` on a stub encoder and a stub VAD."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import hdbscan_grouped_ref as HG  # noqa: E402
import hdbscan_ref as H  # noqa: E402
import launch_log as L  # noqa: E402
from abi_rules import ARG, UNSUP, WS, check_header_and_table, check_versions, refused  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import cluster, hdbscan_gpu  # noqa: E402

HDB = N.PKG_DIR / "csrc" / "hdbscan"
LABEL = re.compile(r'"([a-z0-9_]+_kernel(?:<[^">]*>)?)"')
KKS = (1, 2, 4, 8, 16)

# label -> the function of tests/test_gpu_hdbscan_grouped.py that runs it under expect_launches
_BITWISE = "test_core_and_outgoing_equal_the_ungrouped_kernels_on_every_group"
KERNEL_TESTS = {
    **{f"{kern}<{kk}>": _BITWISE for kern in ("hdb_core_grouped_kernel", "hdb_core_grouped_finish_kernel") for kk in KKS},
    "hdb_outgoing_grouped_kernel": _BITWISE, "hdb_outgoing_grouped_finish_kernel": _BITWISE,
}


def _sources():
    return {f.name: f.read_text() for f in sorted(HDB.glob("*"))}


def _function_text(text, fn):
    m = re.search(rf"^def {fn}\(.*?(?=^\S)", text + "\nend", flags=re.M | re.S)
    return m.group(0) if m else None


# ------------------------------------------------------------------ the census of the directory

def test_every_kernel_of_the_directory_has_one_launch_site_and_literal_labels():
    srcs = _sources()
    assert sorted(srcs) == ["sd_hdb_grouped.hip", "sd_hdb_halves_body.h", "sd_hdb_scan.h", "sd_hdb_scan_body.h"]
    text = "".join(srcs.values())
    kernels = set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", text))
    assert len(kernels) == 4 and all(k.endswith("_kernel") for k in kernels), sorted(kernels)
    labels = set(LABEL.findall(text))
    assert labels == set(KERNEL_TESTS), sorted(labels ^ set(KERNEL_TESTS))
    assert {L.kernel_of(lb) for lb in labels} == kernels
    # one launch site per kernel, each followed by its SD_CHECK_LAUNCH; the templated pair takes its literal from the caller, per KK
    assert len(re.findall(r"\bSD_CHECK_LAUNCH\(", text)) == len(kernels) == len(re.findall(r"\bhipLaunchKernelGGL\(", text))
    assert len(re.findall(r'\bSD_CHECK_LAUNCH\("[a-z0-9_]+_kernel"\)', text)) == 2
    for kk in KKS:
        assert len(re.findall(rf'hg_launch_core<{kk}>\(.*"hdb_core_grouped_kernel<{kk}>", "hdb_core_grouped_finish_kernel<{kk}>"\)', text)) == 1
    # no collision with the census of csrc/*.hip, which stays as it is, nor with the other two directories
    import kernel_census
    assert not kernels & {L.kernel_of(lb) for lb in kernel_census.KERNEL_TESTS}
    for other in ("ahc", "diag"):
        theirs = "".join(f.read_text() for f in sorted((N.PKG_DIR / "csrc" / other).glob("*.hip")))
        assert not kernels & set(re.findall(r"__global__.*?\bvoid\s+([a-z0-9_]+)\s*\(", theirs))


def test_every_label_is_asserted_by_a_gpu_test():
    text = open(os.path.join(HERE, "test_gpu_hdbscan_grouped.py")).read()
    assert "pytestmark = pytest.mark.gpu" in text
    for label, fn in KERNEL_TESTS.items():
        body = _function_text(text, fn)
        assert body, (label, fn)
        assert "expect_launches" in body and L.kernel_of(label) in body, (label, fn)
    # the instantiation comes from _labels(k), which spells it; the test's k cover every KK
    helper = _function_text(text, "_labels")
    assert all(name in helper for name in ("hdb_core_grouped_kernel<", "hdb_core_grouped_finish_kernel<"))
    ks = eval(re.search(r"^KS = (\(.*?\))", text, flags=re.M).group(1))
    assert {1 if k == 1 else 2 if k == 2 else 4 if k <= 4 else 8 if k <= 8 else 16 for k in ks} == set(KKS)
    # the rule bites: a test that never names the kernel is not accepted for it
    body = _function_text(text, "test_a_broken_promise_is_reported")
    assert body and "hdb_outgoing_grouped_finish_kernel" not in body


def test_the_tile_is_the_shared_one_and_nothing_is_atomic():
    """The grouped kernels compute with the tile, the argmax and the slot walk of csrc/sd_gram_tile.h and issue no MFMA of their own
    (so a recording's scores are the bits of the ungrouped entries), nothing in the directory is an atomic, and the top-k insertion and
    the half-tile scan exist once: in the directory's headers, which sd_hdbscan.hip includes as well."""
    text = "".join(_sources().values())
    code = re.sub(r"//.*", "", text)
    assert "atomic" not in code and "__builtin_amdgcn_mfma" not in code
    assert '#include "sd_gram_tile.h"' in code and all(f in code for f in ("gt_tile(", "gt_sym_argmax(", "gt_finish("))
    old = re.sub(r"//.*", "", (N.PKG_DIR / "csrc" / "sd_hdbscan.hip").read_text())
    both = code + old
    assert len(re.findall(r"\bvoid hd_insert\(", both)) == 1 and "void hd_insert(" not in old
    assert len(re.findall(r"\* HD_SC \+ 16 \* j \+ fr\] = acc", both)) == 1 and "HD_SC +" not in old          # the half-tile scan
    for user in (old, _sources()["sd_hdb_grouped.hip"]):
        assert '#include "hdbscan/sd_hdb_scan_body.h"' in user and '#include "hdbscan/sd_hdb_halves_body.h"' in user


def test_the_existing_kernels_are_unchanged_on_record():
    import json
    rec = json.load(open(N.PKG_DIR.parent / "profiles" / "isa_diff_hdb_grouped.json"))
    assert rec["summary"]["differing"] == [] and rec["summary"]["one_side_only"] == [] and rec["summary"]["compile_failed"] == []
    kernels = {L.kernel_of(r["name"].replace("void ", "").split("(")[0]) for r in rec["functions"] if r["kernel"]}
    assert kernels == {"hdb_core_kernel", "hdb_core_finish_kernel", "hdb_outgoing_kernel", "hdb_outgoing_finish_kernel"}
    assert rec["summary"]["kernels"] == 12 and all(r["identical"] for r in rec["functions"])


# ------------------------------------------------------------------ ABI

NEW = {"sd_hdb_core_grouped_workspace_bytes", "sd_hdb_core_grouped_f32", "sd_hdb_outgoing_grouped_workspace_bytes", "sd_hdb_outgoing_grouped_f32"}


def test_header_and_binding_table_name_the_same_exported_entries():
    names = check_header_and_table("sd_hip_hdbscan.h", N.HDBSCAN_PROTOTYPES,
                                   (N.PROTOTYPES, N.SPECTRAL_PROTOTYPES, N.AHC_PROTOTYPES, N.DIAG_PROTOTYPES, N.TRACE_PROTOTYPES))
    assert names == NEW | {"sd_hdbscan_abi_version", "sd_hdb_core_workspace_bytes", "sd_hdb_core_f32", "sd_hdb_outgoing_workspace_bytes",
                           "sd_hdb_outgoing_f32"}
    from speech_diarization_amd import ops
    assert NEW <= ops._ENTRIES                                        # through the table they reach `ops.launch` by themselves


def test_every_abi_version_is_untouched():
    """The four entries are additive: the header says that such entries do not move the version."""
    assert N.SD_HDBSCAN_ABI_VERSION == 1
    check_versions(sd_ahc_abi_version=1, sd_abi_version=11, sd_spectral_abi_version=1, sd_hdbscan_abi_version=1, sd_diag_abi_version=1,
                   sd_trace_abi_version=3)
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_hdbscan.h").read()
    assert re.search(r"#define\s+SD_HDBSCAN_ABI_VERSION\s+1\b", header)
    assert re.search(r"additive entry[^.]*does not move it", re.sub(r"\s*\n \*\s*", " ", header))


NS = (1, 127, 128, 129, 1000, 50000)


def test_workspace_formulas():
    """Core: ceil((2 W + 1) / 8) slots of k scores per padded row.  Outgoing: (2 W + 2) slots of a weight and an index per padded row,
    the grouped AHC entry's.  W = min(T - 1, ceil((max_group - 1) / 128)), T = ceil(n / 128); d does not enter beyond its range."""
    lib = N.load()
    core, out = lib.sd_hdb_core_grouped_workspace_bytes, lib.sd_hdb_outgoing_grouped_workspace_bytes
    header = open(N.PKG_DIR.parent / "include" / "sd_hip_hdbscan.h").read()
    assert "ceil((2 W + 1) / 8) · 128 T · k · 4" in header and "(2 W + 2) · 128 T · 8" in header
    for n in NS:
        t = -(-n // 128)
        for max_group in (1, 2, 128, 129, 1000, n):
            w = min(t - 1, -(-(max_group - 1) // 128))
            for d in (1, 190, 1024):
                assert int(out(n, d, max_group)) == (2 * w + 2) * 128 * t * 8 == HG.outgoing_workspace_bytes(n, max_group), (n, d, max_group)
                assert int(out(n, d, max_group)) == int(lib.sd_ahc_nearest_grouped_workspace_bytes(n, d, max_group))
                for k in (1, 3, 16):
                    want = -(-(2 * w + 1) // 8) * 128 * t * k * 4
                    assert int(core(n, d, k, max_group)) == want == HG.core_workspace_bytes(n, k, max_group), (n, d, k, max_group)
    assert int(core(128, 192, 1, 128)) == 512 and int(core(129, 192, 3, 1)) == 2 * 128 * 3 * 4 and int(core(1000, 192, 16, 500)) == 2 * 1024 * 64
    # no k <= n - 1 rule: a group smaller than k + 1 is legal and gives -inf
    assert int(core(1, 192, 16, 1)) == 128 * 16 * 4 and int(lib.sd_hdb_core_workspace_bytes(1, 192, 16)) == 0
    assert int(core(1000, 192, 2, 2 ** 31 - 1)) == int(core(1000, 192, 2, 1000))               # max_group above n changes nothing
    # one group over everything: the band is every tile, and the slots are those of the ungrouped core pass wherever 2 T - 1 <= 8
    for n in (129, 500):
        assert int(core(n, 192, 2, n)) == int(lib.sd_hdb_core_workspace_bytes(n, 192, 2))
    for args in ((0, 192, 2, 5), (-3, 192, 2, 5), (100, 0, 2, 5), (100, -1, 2, 5), (100, 1025, 2, 5), (100, 192, 0, 5), (100, 192, -1, 5),
                 (100, 192, 17, 5), (100, 192, 2, 0), (100, 192, 2, -7)):
        assert int(core(*args)) == 0, args
    for args in ((0, 192, 5), (-3, 192, 5), (100, 0, 5), (100, -1, 5), (100, 1025, 5), (100, 192, 0), (100, 192, -7)):
        assert int(out(*args)) == 0, args


def test_workspaces_grow_linearly_in_n():
    """At max_group = 500 (W = 4 once T > 4: 9 column tiles, 2 chunks; 10 slots) doubling n doubles the bytes to within one tile row."""
    lib = N.load()
    core, out = lib.sd_hdb_core_grouped_workspace_bytes, lib.sd_hdb_outgoing_grouped_workspace_bytes
    for n in (1000, 4000, 16001, 64000, 250000):
        for fn, row in ((lambda m: int(core(m, 192, 3, 500)), 2 * 128 * 3 * 4), (lambda m: int(out(m, 192, 500)), 10 * 128 * 8)):
            one, two = fn(n), fn(2 * n)
            assert abs(two - 2 * one) <= row and one <= (n + 127) * row // 128, (n, one, two)
    assert int(lib.sd_hdb_core_workspace_bytes(250000, 192, 3)) > 100 * int(core(250000, 192, 3, 500))        # the full walk is quadratic
    assert int(lib.sd_hdb_outgoing_workspace_bytes(250000, 192)) > 100 * int(out(250000, 192, 500))


# ------------------------------------------------------------------ refusals before launch (no device needed: fake non-null pointers)

def _core(lib, rows=0x1000, ld=192, n=100, d=192, k=2, group=0x6000, max_group=40, core=0x2000, bad=0x7000, ws=0x5000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = int(lib.sd_hdb_core_grouped_workspace_bytes(n, d, k, max_group)) if n > 0 else 0
    return lib.sd_hdb_core_grouped_f32(rows, ld, n, d, k, group, max_group, core, bad, ws, ws_bytes, None)


def _outgoing(lib, rows=0x1000, ld=192, n=100, d=192, core=0x2000, comp=0x8000, group=0x6000, max_group=40, nn=0x3000, best=0x4000,
              bad=0x7000, ws=0x5000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = int(lib.sd_hdb_outgoing_grouped_workspace_bytes(n, d, max_group)) if n > 0 else 0
    return lib.sd_hdb_outgoing_grouped_f32(rows, ld, n, d, core, comp, group, max_group, nn, best, bad, ws, ws_bytes, None)


def test_refusals_happen_before_anything_is_launched():
    """Every case returns its own argument / support / workspace code with a message.  A launch on this pointer soup would have
    returned SD_ERR_HIP (no device here) or faulted (on a GPU)."""
    lib = N.load()
    for name in ("rows", "group", "core", "bad", "ws"):
        refused(_core(lib, **{name: None}), ARG, "null pointer")
    for name in ("rows", "core", "comp", "group", "nn", "best", "bad", "ws"):
        refused(_outgoing(lib, **{name: None}), ARG, "null pointer")
    for call, who in ((_core, "sd_hdb_core_grouped_f32"), (_outgoing, "sd_hdb_outgoing_grouped_f32")):
        refused(call(lib, n=0), ARG, "n=0")
        refused(call(lib, n=-5), ARG, "n=-5")
        refused(call(lib, d=0), ARG, "d=0")
        refused(call(lib, d=-1), ARG, "d=-1")
        refused(call(lib, d=192, ld=188), ARG, "ld=188")
        refused(call(lib, rows=0x1004), ARG, "rows must be 16-byte aligned")
        refused(call(lib, rows=0x1008), ARG, "16-byte aligned")
        refused(call(lib, d=190, ld=190), ARG, "ld=190")
        refused(call(lib, d=7, ld=9), ARG, "ld=9")
        refused(call(lib, max_group=0, ws_bytes=1 << 20), ARG, "max_group=0")
        refused(call(lib, max_group=-3, ws_bytes=1 << 20), ARG, "max_group=-3")
        assert N.last_error().startswith(who + ": ")
        refused(call(lib, d=1025, ld=1028, ws_bytes=1 << 30), UNSUP, "d=1025")
        refused(call(lib, ws=0x5004), ARG, "workspace is not 16-byte aligned")
        refused(call(lib, ws_bytes=0), WS, "workspace of 0 bytes")
    refused(_core(lib, k=17, ws_bytes=1 << 30), UNSUP, "k=17, at most 16 neighbours")
    refused(_core(lib, k=0, ws_bytes=1 << 30), ARG, "k=0 must be at least 1")
    refused(_core(lib, k=-1, ws_bytes=1 << 30), ARG, "k=-1")
    assert _core(lib, n=0, k=0, max_group=0, rows=None) == ARG and "n=0 d=192 ld=192" in N.last_error()       # precedence: the shape first,
    refused(_core(lib, d=1025, ld=1028, k=17, max_group=0, rows=None), UNSUP, "d=1025")                         # then d, then k (support
    refused(_core(lib, k=17, max_group=0, rows=None), UNSUP, "k=17")                                           # before argument, as the
    refused(_core(lib, k=0, max_group=0, rows=None), ARG, "k=0")                                               # ungrouped entry), then
    refused(_core(lib, max_group=0, rows=None), ARG, "max_group=0")                                            # max_group, the pointers,
    refused(_core(lib, rows=None, d=190, ld=190, ws=0x5004), ARG, "null pointer")                              # the rows' alignment, the
    refused(_core(lib, ld=190, d=190, ws=0x5004, ws_bytes=0), ARG, "ld=190")                                   # workspace's, the grid
    refused(_core(lib, ws=0x5004, ws_bytes=0), ARG, "workspace is not")                                        # limit and the size
    refused(_core(lib, n=128 * 65535 + 1, max_group=5, ws_bytes=0), UNSUP, "at most 8388480 rows")
    refused(_outgoing(lib, max_group=0, rows=None), ARG, "max_group=0")
    refused(_outgoing(lib, rows=None, d=190, ld=190, ws=0x5004), ARG, "null pointer")
    need = int(lib.sd_hdb_core_grouped_workspace_bytes(100, 192, 2, 40))
    refused(_core(lib, ws_bytes=need - 1), WS, f"workspace of {need - 1} bytes, n=100 d=192 k=2 max_group=40 needs {need}")
    need = int(lib.sd_hdb_outgoing_grouped_workspace_bytes(100, 192, 40))
    refused(_outgoing(lib, ws_bytes=need - 1), WS, f"workspace of {need - 1} bytes, n=100 d=192 max_group=40 needs {need}")
    # the workspace of a smaller bound, or of a smaller k, does not serve a larger one
    refused(_core(lib, n=3000, max_group=1500, ws_bytes=int(lib.sd_hdb_core_grouped_workspace_bytes(3000, 192, 2, 129))), WS, "max_group=1500")
    refused(_core(lib, k=3, ws_bytes=int(lib.sd_hdb_core_grouped_workspace_bytes(100, 192, 2, 40))), WS, "k=3")
    refused(_outgoing(lib, n=1000, max_group=500, ws_bytes=int(lib.sd_hdb_outgoing_grouped_workspace_bytes(1000, 192, 129))), WS, "max_group=500")


def test_the_entries_refuse_through_the_one_check():
    """Both entries and both size functions go through csrc/sd_rows_check.h (`sd_rows_refused`, `sd_rows_workspace_bytes`); the file has
    no argument check of its own.  The new kind stands at the END of SdRowsKind and the new field at the end of SdRowsCall: the eight
    earlier descriptions compile and behave as before (tests/test_rows_check_rules.py builds them from tests/helpers/rows_check_pure.cpp)."""
    code = re.sub(r"//[^\n]*", "", (HDB / "sd_hdb_grouped.hip").read_text())
    assert not re.search(r"\bSD_CHECK_ARG\(|\bsd_set_error\(", code)
    assert len(re.findall(r"\bsd_rows_refused\(", code)) == 2 and len(re.findall(r"\bsd_rows_workspace_bytes\(", code)) == 2
    check = (N.PKG_DIR / "csrc" / "sd_rows_check.h").read_text()
    kinds = re.search(r"enum SdRowsKind \{([^}]*)\}", check).group(1).replace(" ", "").split(",")
    assert kinds == ["SD_ROWS_ONLY", "SD_ROWS_LABELS", "SD_ROWS_SYM", "SD_ROWS_BAND", "SD_ROWS_CORE", "SD_ROWS_WHITEN", "SD_ROWS_BAND_CORE"]
    fields = re.search(r"struct SdRowsCall \{(.*?)\n\};", check, flags=re.S).group(1)
    assert re.sub(r"//[^\n]*", "", fields).strip().endswith("size_t ws_bytes;\n  int max_group;")


def test_wrappers_and_route_have_no_cpu_fallback():
    from speech_diarization_amd import anti_stick_diarize as asd, ops
    S, g = torch.ones(4, 8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hdb_core_grouped(S, 1, g, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hdb_outgoing_grouped(S, torch.ones(4), g, g, 4)
    X = H.planted(40, 2, 0.5, 0, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hdbscan_gpu.hdbscan_rows_groups(torch.from_numpy(X), [30, 10])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hdbscan_gpu.hdbscan_rows_groups(X, [30, 10])
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            hdbscan_gpu.HdbscanGpuClusterer().fit_predict_many([X, X])
    for other in ("hdbscan_two_stage", "ahc", "ahc_affinity", cluster.default_hdbscan_factory):
        with pytest.raises(ValueError, match="hdbscan_gpu"):
            asd.diarize_many([np.zeros(16000, np.float32)], clusterer=other)
    assert callable(asd.cluster_hdbscan_two_stage_many)                                                   # re-exported under the reference's module


# ------------------------------------------------------------------ the numpy statement of the entries

def test_numpy_statement_masks_groups_and_components():
    rng = np.random.default_rng(3)
    X = H.unit_rows(rng.standard_normal((300, 16)))
    X[[3, 10, 140, 141, 290]] = X[3]                                    # the largest score there is, inside and across groups
    sizes = [100, 1, 150, 49]
    group = HG.group_of(sizes)
    G = H.gram_f32(X)
    core = HG.core_grouped_from_gram(G, 2, group)
    assert core[100] == -np.inf and np.isfinite(np.delete(core, 100)).all()
    assert np.array_equal(core[:100], H.core_from_gram(G[:100, :100], 2)) and np.array_equal(core[251:], H.core_from_gram(G[251:, 251:], 2))
    assert HG.core_grouped_from_gram(G, 49, group)[251:].tolist() == [-np.inf] * 49                       # 48 others: fewer than k
    inf = np.full(300, np.inf, np.float32)
    nn, best = HG.outgoing_grouped_from_gram(G, inf, np.arange(300), group)
    assert nn[3] == 10 and nn[10] == 3 and nn[140] == 141 and nn[141] == 140 and nn[100] == -1 and best[100] == -np.inf
    assert group[nn[290]] == 3 and best[290] < 0.99
    assert all(group[nn[i]] == group[i] for i in range(300) if i != 100)
    comp = np.arange(300)
    comp[10] = comp[3]                                                  # rows 3 and 10 in one component: no edge between them any more
    nn2, best2 = HG.outgoing_grouped_from_gram(G, inf, comp, group)
    assert nn2[3] != 10 and nn2[10] != 3 and best2[3] < best[3] and nn2[140] == 141
    one = np.zeros(300, np.int64)                                       # everything one component: no edge at all
    assert (HG.outgoing_grouped_from_gram(G, inf, one, group)[0] == -1).all()
    assert not HG.promise_broken(group, 150) and HG.promise_broken(group, 149)


# ------------------------------------------------------------------ the driver on the CPU

@pytest.fixture(scope="module")
def folder():
    """The recordings, their rows in one matrix, one operator over them (its Gram is formed once), and the lone runs, formed once per
    (recording, setting, metric): `hdbscan_rows` with an operator that reads the recording's block of the same Gram."""
    recs = HG.driver_recordings()
    X = np.concatenate([x for _, x in recs])
    op = HG.NumpyGroupedRows()
    rows = op.normalise(torch.from_numpy(X))
    op.normalise = lambda _X: rows                                      # the same tensor every call: one Gram
    bounds = np.concatenate([[0], np.cumsum([len(x) for _, x in recs])])
    cache = {}

    def alone(i, setting, metric):
        if (i, setting, metric) not in cache:
            a, b = int(bounds[i]), int(bounds[i + 1])
            lone = op.alone(rows, a, b)
            lone.normalise = lambda _X: rows[a:b]
            mcs, ms, single = setting
            cache[i, setting, metric] = hdbscan_gpu.hdbscan_rows(torch.from_numpy(X[a:b]), mcs, ms, single, metric, operator=lone, return_info=True)
        return cache[i, setting, metric]
    return recs, X, op, alone


def _admits(size, setting):
    mcs, ms, _ = setting
    return size < 2 or (ms or mcs) <= size


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("setting", H.SETTINGS)
def test_groups_equal_every_recording_alone_exactly(folder, setting, metric):
    """The claim of DESIGN.md section 20: per recording the labels are those of `hdbscan_rows` on the recording alone, EXACTLY, ties or
    no ties (the recorded tie input and a recording of identical rows are in the folder), because the same edge array reaches the same
    scikit-learn routines.  The rounds are the maximum of the lone runs' rounds, and the operator saw max-many passes, not sum-many."""
    recs, X, op, alone = folder
    names = [name for name, _ in recs]
    assert [len(x) for _, x in recs] == [300, 2, 0, 1000, 1, 3, 40, 129, 700] and "tied1000" in names and "identical40" in names
    keep = [i for i, (_, x) in enumerate(recs) if _admits(len(x), setting)]
    assert {len(recs[i][1]) for i in keep} >= {0, 1, 300, 1000, 129, 700} and (setting != (2, None, True) or len(keep) == len(recs))
    sizes = [len(recs[i][1]) for i in keep]
    bounds = np.concatenate([[0], np.cumsum([len(x) for _, x in recs])])
    sub = HG.NumpyGroupedRows()
    Xs = np.concatenate([recs[i][1] for i in keep])
    if len(keep) == len(recs):
        sub, before = op, op.passes
    else:                                                               # a folder without the recordings this setting does not admit
        idx = np.concatenate([np.arange(bounds[i], bounds[i + 1]) for i in keep]).astype(int)
        G = op._G(op.normalise(None))[np.ix_(idx, idx)]
        sub._G = lambda rows: G
        before = 0
    mcs, ms, single = setting
    labels, info = hdbscan_gpu.hdbscan_rows_groups(torch.from_numpy(Xs), sizes, mcs, ms, single, metric, operator=sub, return_info=True)
    want = [alone(i, setting, metric) for i in keep]
    assert len(labels) == len(keep)
    for i, got, (lab, inf) in zip(keep, labels, want):
        assert got.dtype.kind == "i" and got.shape == lab.shape and np.array_equal(got, lab), (names[i], int((got != lab).sum()))
    assert info["mst_weight"] == [inf["mst_weight"] for _, inf in want]
    rounds = [inf["rounds"] for _, inf in want]
    assert info["rounds"] == max(rounds) <= int(np.ceil(np.log2(max(sizes))))
    core_passes = 1 if (ms or mcs) > 1 else 0
    assert sub.passes - before == max(rounds) + core_passes < sum(r + core_passes for r in rounds)
    assert info["components_per_round"][-1] == sum(1 for s in sizes if s) and len(info["components_per_round"]) == max(rounds)
    print(f"{setting} {metric}: rounds alone {rounds}, together {info['rounds']}; gram_tiles {info['gram_tiles']} {info['gram_tiles_per_pass']}")


def _reachable(sizes):
    """(diagonal tiles, tiles I < J that hold two rows of one recording), counted from the statement."""
    group = HG.group_of(sizes)
    T = -(-len(group) // 128)
    blocks = [set(group[128 * t:128 * t + 128].tolist()) for t in range(T)]
    return T, sum(1 for i in range(T) for j in range(i + 1, T) if blocks[i] & blocks[j])


def test_gram_tiles_are_the_tiles_a_recording_reaches():
    rng = np.random.default_rng(0)
    for sizes in ([300] * 7, [1, 2, 5, 127, 128, 129, 257] + [3] * 40 + [1000, 1], [128, 128, 128], [5], [700, 1, 0, 90]):
        X = H.unit_rows(rng.standard_normal((sum(sizes), 8)))
        _, info = hdbscan_gpu.hdbscan_rows_groups(torch.from_numpy(X), sizes, 2, 2, operator=HG.NumpyGroupedRows(), return_info=True)
        diagonal, above = _reachable(sizes)
        assert info["gram_tiles_per_pass"] == [diagonal + 2 * above] + [diagonal + above] * info["rounds"], sizes
        assert info["gram_tiles"] == sum(info["gram_tiles_per_pass"])
        T, W = HG.band(sum(sizes), max(sizes))
        assert diagonal + above <= T * (W + 1) and diagonal + 2 * above <= T * (2 * W + 1)
        _, info1 = hdbscan_gpu.hdbscan_rows_groups(torch.from_numpy(X), sizes, 2, 1, operator=HG.NumpyGroupedRows(), return_info=True)
        assert info1["gram_tiles_per_pass"] == [diagonal + above] * info1["rounds"]              # min_samples = 1: no core pass


def test_tiny_and_refused_inputs():
    class Untouchable:
        device = torch.device("cpu")

        def __getattr__(self, name):
            raise AssertionError(f"operator.{name} reached")
    rows_groups = hdbscan_gpu.hdbscan_rows_groups
    labels, info = rows_groups(torch.zeros(3, 4), [1, 0, 1, 1], operator=Untouchable(), return_info=True)
    assert [lab.tolist() for lab in labels] == [[0], [], [0], [0]] and all(lab.dtype.kind == "i" for lab in labels)
    assert info["rounds"] == 0 and info["gram_tiles"] == 0 and info["components_per_round"] == []
    assert rows_groups(torch.zeros(0, 4), [], operator=Untouchable()) == []
    X = np.concatenate([H.planted(100, 2, 0.5, 0, 0), H.planted(300, 3, 0.5, 1, 0)])
    for bad in (np.nan, np.inf):
        Xb = X.copy()
        Xb[117, 3] = bad
        for metric in ("euclidean", "cosine"):
            with pytest.raises(ValueError, match="recording 1: rows must be finite"):
                rows_groups(torch.from_numpy(Xb), [100, 300], metric=metric, operator=Untouchable())
    for scale in (0.0, 0.99, 1.01, 3.0):
        Xb = X.copy()
        Xb[5] *= np.float32(scale)
        with pytest.raises(ValueError, match="recording 0: metric 'euclidean' takes unit rows"):
            rows_groups(torch.from_numpy(Xb), [100, 300], operator=Untouchable())
    with pytest.raises(ValueError, match=r"recording 2: min_samples \(6\) must be at most the number of rows \(5\)"):
        rows_groups(torch.from_numpy(X), [100, 1, 5, 294], 2, 6, operator=Untouchable())
    with pytest.raises(ValueError, match="add up"):
        rows_groups(torch.from_numpy(X), [100, 299], operator=Untouchable())
    with pytest.raises(ValueError, match="add up"):
        rows_groups(torch.from_numpy(X), [500, -100], operator=Untouchable())
    with pytest.raises(ValueError, match="min_cluster_size"):
        rows_groups(torch.from_numpy(X), [100, 300], 1, operator=Untouchable())
    with pytest.raises(ValueError, match="metric"):
        rows_groups(torch.from_numpy(X), [100, 300], metric="precomputed", operator=Untouchable())
    # the two rows of tests/test_hdbscan_rules.py between two singletons
    two = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0]], np.float32)
    got, info = rows_groups(torch.from_numpy(np.concatenate([two[:1], two, two[1:]])), [1, 2, 1], operator=HG.NumpyGroupedRows(), return_info=True)
    assert [g.tolist() for g in got] == [[0], [0, 0], [0]] and info["rounds"] == 1


def test_a_broken_promise_raises():
    """An operator whose kernel reports `bad` stops the driver: from the core pass (read with the first round) and from a round."""
    class LyingCore(HG.NumpyGroupedRows):
        def core_grouped(self, rows, k, group, max_group):
            return super().core_grouped(rows, k, group, max_group - 1)

    class LyingRound(HG.NumpyGroupedRows):
        def outgoing_grouped(self, rows, core, comp, group, max_group):
            return super().outgoing_grouped(rows, core, comp, group, max_group - 1)
    X = torch.from_numpy(np.concatenate([H.planted(100, 2, 0.5, 0, 0), H.planted(300, 3, 0.5, 1, 0)]))
    for op in (LyingCore(), LyingRound()):
        with pytest.raises(RuntimeError, match="max_group=300"):
            hdbscan_gpu.hdbscan_rows_groups(X, [100, 300], operator=op)

    class Unmasked(HG.NumpyGroupedRows):                                # an operator that forgets the group mask
        def outgoing_grouped(self, rows, core, comp, group, max_group):
            return super().outgoing_grouped(rows, core, comp, torch.zeros_like(group), len(group))
    with pytest.raises((RuntimeError, AssertionError), match="mask is wrong"):
        hdbscan_gpu.hdbscan_rows_groups(X, [100, 300], operator=Unmasked())


# ------------------------------------------------------------------ the two-stage glue

def _glue_recordings():
    """Conversations (one scaled away from unit norm), and the early exits of the glue: no rows, one row, two rows, and one tight
    cluster (a single centroid: fewer than min_cluster_size)."""
    rng = np.random.default_rng(4)
    a, b = H.planted(300, 4, 0.6, 0, 0), H.planted(129, 3, 0.5, 5, 4)
    tight = H.unit_rows(HG.identical_rows(6) + 1e-3 * rng.standard_normal((6, 192)).astype(np.float32))
    return [a * np.float32(3.0), a[:0], b, a[5:6], tight, b[:2], H.planted(700, 3, 0.5, 1, 0)]


def test_two_stage_many_equals_two_stage_per_recording():
    """With the numpy-operator clusterer (`fit_predict_many`: stage 1 is ONE call over all recordings, stage 2 ONE over all centroids)
    and with scikit-learn's (no `fit_predict_many`: the loop path)."""
    every = _glue_recordings()
    made = []

    class Counting(hdbscan_gpu.HdbscanGpuClusterer):
        def fit_predict_many(self, mats):
            made.append([len(m) for m in mats])
            return super().fit_predict_many(mats)

    def factory(**kw):
        return Counting(kw["min_cluster_size"], kw["min_samples"], kw["allow_single_cluster"], kw["metric"], operator=HG.NumpyGroupedRows())
    for mcs in (2, 5):
        recs = [x for x in every if len(x) < 2 or len(x) >= mcs]      # a clusterer refuses min_samples above the rows, alone as together
        assert len(recs) == (7 if mcs == 2 else 6)
        made.clear()
        got = cluster.cluster_hdbscan_two_stage_many(recs, mcs, clusterer_factory=factory)
        want = [cluster.cluster_hdbscan_two_stage(x, mcs, clusterer_factory=hdbscan_gpu.HdbscanGpuClusterer.factory(operator=H.NumpyRows())) for x in recs]
        assert len(got) == len(recs)
        for x, g, w in zip(recs, got, want):
            assert g.shape == w.shape and g.dtype == w.dtype and H.same_clustering(g, w) and np.array_equal(g, w), len(x)
        # one call per stage; at min_cluster_size = 5 every recording has fewer than 5 centroids and none reaches stage 2
        assert len(made) == (2 if mcs == 2 else 1) and made[0] == [len(x) for x in recs if len(x) >= 2], made
        assert got[1].tolist() == [] and got[1].dtype == np.array([]).dtype and got[3].tolist() == [0]
    recs = every
    loop = cluster.cluster_hdbscan_two_stage_many(recs, 2)
    for x, g in zip(recs, loop):
        w = cluster.cluster_hdbscan_two_stage(x, 2)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), len(x)
    assert cluster.cluster_hdbscan_two_stage_many([]) == []
    from speech_diarization_amd import anti_stick_diarize as asd
    again = asd.cluster_hdbscan_two_stage_many(recs, 2)
    assert all(np.array_equal(p, q) for p, q in zip(again, loop))


# ------------------------------------------------------------------ the public interface

def _fft_encoder(w):
    return np.stack([np.abs(np.fft.rfft(r, 382))[:192] for r in np.asarray(w, dtype=np.float32)]).astype(np.float32)


def _vad(y, sr, **kw):
    if not np.any(y):
        return []
    return [(0.5 * i, 0.5 * i + 0.45) for i in range(int(len(y) / sr / 0.5))]


def _triples(segs):
    return [(s.start, s.end, s.spk) for s in segs]


def test_diarize_many_equals_diarize_per_recording(monkeypatch):
    """Stub encoder and stub VAD, as tests/test_hdbscan_rules.py does for `diarize`; the product factory is patched to the numpy
    operator.  A conversation, a silent recording, a second conversation, one with a single segment."""
    from speech_diarization_amd import anti_stick_diarize as asd
    from speech_diarization_amd import synth
    ys = [synth.synthetic_conversation(20.0, 2, seed=0).wav, np.zeros(3 * 16000, np.float32), synth.synthetic_conversation(12.0, 3, seed=1).wav,
          synth.synthetic_conversation(20.0, 2, seed=0).wav[:int(0.9 * 16000)]]
    kw = dict(encode=_fft_encoder, vad_segments=_vad, scd_thr=1e9)
    default = [asd.diarize(y, **kw) for y in ys]                          # default arguments of everything else, before any patch
    product_factory = hdbscan_gpu.HdbscanGpuClusterer.factory
    calls = []

    def factory(operator=None):
        assert operator is None
        calls.append(1)
        return product_factory(operator=HG.NumpyGroupedRows())
    monkeypatch.setattr(hdbscan_gpu.HdbscanGpuClusterer, "factory", staticmethod(factory))
    for reseg in (0, 1):
        want = [asd.diarize(y, **kw, reseg=reseg, clusterer="hdbscan_gpu") for y in ys]
        calls.clear()
        got = asd.diarize_many(ys, **kw, reseg=reseg)
        assert len(calls) == 1                                            # ONE two-stage call for the folder
        assert [_triples(g) for g in got] == [_triples(w) for w in want]
        assert got[1] == [] and len(got[0]) >= 1 and len(got[3]) == 1 and len({s.spk for s in got[0]}) >= 1
    assert asd.diarize_many([], **kw) == []
    # `diarize` with default arguments on the same stubs: the default clusterer (scikit-learn's) is untouched by the patch
    again = [asd.diarize(y, **kw) for y in ys]
    assert [_triples(a) for a in again] == [_triples(d) for d in default]
    import inspect
    p_one, p_many = inspect.signature(asd.diarize).parameters, inspect.signature(asd.diarize_many).parameters
    assert list(p_many)[1:] == list(p_one)[1:] and list(p_many)[0] == "wav_paths"
    assert all(p_many[k].default == p_one[k].default and p_many[k].kind == p_one[k].kind for k in list(p_one)[1:] if k != "clusterer")
    assert p_many["clusterer"].default == "hdbscan_gpu" and p_one["clusterer"].default == "hdbscan_two_stage"


def test_build_list_and_fingerprint_cover_the_directory():
    import importlib.util
    spec = importlib.util.spec_from_file_location("sd_build_native_hdb", str(N.PKG_DIR / "build_native.py"))
    bn = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bn)
    assert "hdbscan/sd_hdb_grouped.hip" in bn.SOURCES and all((bn.CSRC / s).exists() for s in bn.SOURCES)
    assert len({os.path.basename(s) for s in bn.SOURCES}) == len(bn.SOURCES)             # object files are named by the stem
    src = (N.PKG_DIR / "build_native.py").read_text()
    assert '(CSRC / "hdbscan").glob' in _function_text(src, "_fingerprint")
