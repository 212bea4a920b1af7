"""No-GPU checks of the device HDBSCAN route (include/sd_hip_hdbscan.h, speech-diarization_amd/hdbscan_gpu.py): the binding table, the
workspace formulas, the refusals an entry makes before it launches anything, and the driver itself run on the CPU through an injected
numpy operator against an f64 Prim tree and against scikit-learn's HDBSCAN.

The label table holds 16 of the 48 combinations of hdbscan_ref.SHAPES x SETTINGS x seeds 0 .. 2.  45 of the 48 agree with the host.
The three that do not are one input, planted(1000, 8, 0.8, seed 2, 20 outliers), at the three settings with min_samples >= 3, and one
row of it: row 2 hangs on the spanning tree by two edges of exactly equal weight (its own core value), so which sub-tree it joins
first is an accident of the order in which the two edges reach scikit-learn's linkage routine (hdbscan_ref.TIED_INPUT; the caveat of the
module docstring of hdbscan_gpu.py).  (6, 3, False) differs under both metrics, hdbscan_ref.RECORDED_NEAR_TIE; (5, None, True) and
(15, 5, True) under "cosine" only.  That input is in no table; test_the_recorded_tie_is_a_property_of_the_input states the tie."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import hdbscan_ref as H  # noqa: E402
from abi_rules import ARG, UNSUP, WS, check_header_and_table, check_versions, refused  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import cluster  # noqa: E402

needs_lib = pytest.mark.skipif(not N.LIB_PATH.exists(), reason="libsd_hip.so is not built")


def _route():
    from speech_diarization_amd import hdbscan_gpu
    return hdbscan_gpu


# ------------------------------------------------------------------ ABI

@needs_lib
def test_header_and_binding_table_name_the_same_exported_entries():
    check_header_and_table("sd_hip_hdbscan.h", N.HDBSCAN_PROTOTYPES, (N.PROTOTYPES, N.SPECTRAL_PROTOTYPES, N.AHC_PROTOTYPES))


@needs_lib
def test_versions():
    assert N.SD_HDBSCAN_ABI_VERSION == 1
    check_versions(sd_hdbscan_abi_version=1, sd_abi_version=11, sd_spectral_abi_version=1, sd_ahc_abi_version=1)      # the others: untouched


@needs_lib
def test_workspace_formulas():
    """outgoing: (T + 1) slots of 128 T padded rows, a weight and an index each (the AHC formula).  core: ceil(T / 8) slots of 128 T
    padded rows, k scores each.  d does not enter beyond its range."""
    lib = N.load()
    for n in (1, 2, 5, 127, 128, 129, 257, 1000, 1025, 7609, 50000):
        t = -(-n // 128)
        for d in (1, 7, 190, 192, 1024):
            assert int(lib.sd_hdb_outgoing_workspace_bytes(n, d)) == (t + 1) * t * 128 * 8 == int(lib.sd_ahc_nearest_workspace_bytes(n, d)), (n, d)
            for k in (1, 2, 3, 16):
                want = -(-t // 8) * t * 128 * k * 4 if k <= n - 1 else 0
                assert int(lib.sd_hdb_core_workspace_bytes(n, d, k)) == want, (n, d, k)
    assert int(lib.sd_hdb_core_workspace_bytes(128, 192, 1)) == 512 and int(lib.sd_hdb_core_workspace_bytes(1025, 192, 2)) == 2 * 9 * 128 * 2 * 4
    for n, d in ((0, 192), (-3, 192), (100, 0), (100, -1), (100, 1025)):
        assert int(lib.sd_hdb_outgoing_workspace_bytes(n, d)) == 0, (n, d)
    for n, d, k in ((0, 192, 1), (1, 192, 1), (-3, 192, 1), (100, 0, 1), (100, 1025, 1), (100, 192, 0), (100, 192, -1), (100, 192, 17),
                    (10, 192, 10), (2, 192, 2)):
        assert int(lib.sd_hdb_core_workspace_bytes(n, d, k)) == 0, (n, d, k)


# ------------------------------------------------------------------ one statement of the tile

def test_the_gram_tile_is_stated_once():
    """`<a, b>` and `<b, a>` are the same bits in the AHC and the HDBSCAN kernels because both call the tile, the loads and the
    tie rule of csrc/sd_gram_tile.h: neither file issues the f32 MFMA itself or defines a `load4` / `take` of its own.  sd_affinity.hip,
    whose exact-f32 step stages differently and legitimately has its own, shows that the search finds the builtin where it is."""
    csrc = N.PKG_DIR / "csrc"
    mfma = "__builtin_amdgcn_mfma_f32_16x16x4f32"
    own = re.compile(r"^[^\n;]*\b\w*(?:load4|take)\s*\([^;{]*\)\s*\{", re.M)      # a definition, not a call
    header = (csrc / "sd_gram_tile.h").read_text()
    assert mfma in header and "__global__" not in header
    assert {m.group(0).split("(")[0].split()[-1] for m in own.finditer(header)} == {"gt_load4", "gt_take"}
    for name in ("sd_ahc.hip", "sd_hdbscan.hip"):
        text = (csrc / name).read_text()
        assert mfma not in text, name
        assert not own.search(text), (name, own.search(text).group(0))
        assert '#include "sd_gram_tile.h"' in text and "gt_tile(" in text, name
    assert mfma in (csrc / "sd_affinity.hip").read_text()


# ------------------------------------------------------------------ refusals before launch (no device needed: fake non-null pointers)

def _core(lib, rows=0x1000, ld=192, n=100, d=192, k=2, core=0x2000, ws=0x5000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = int(lib.sd_hdb_core_workspace_bytes(n, d, k))
    return lib.sd_hdb_core_f32(rows, ld, n, d, k, core, ws, ws_bytes, None)


def _outgoing(lib, rows=0x1000, ld=192, n=100, d=192, core=0x2000, comp=0x3000, nn=0x4000, best=0x6000, ws=0x5000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = int(lib.sd_hdb_outgoing_workspace_bytes(n, d))
    return lib.sd_hdb_outgoing_f32(rows, ld, n, d, core, comp, nn, best, ws, ws_bytes, None)


@needs_lib
def test_refusals_happen_before_anything_is_launched():
    """Every case returns its own argument / support / workspace code with a message.  A launch on this pointer soup would have
    returned SD_ERR_HIP (no device here) or faulted (on a GPU)."""
    lib = N.load()
    for name in ("rows", "core", "ws"):
        refused(_core(lib, **{name: None}), ARG, "null pointer")
    for name in ("rows", "core", "comp", "nn", "best", "ws"):
        refused(_outgoing(lib, **{name: None}), ARG, "null pointer")
    for call, who in ((_core, "sd_hdb_core_f32"), (_outgoing, "sd_hdb_outgoing_f32")):
        refused(call(lib, n=0, ws_bytes=1 << 20), ARG, "n=0")
        refused(call(lib, n=-5, ws_bytes=1 << 20), ARG, "n=-5")
        refused(call(lib, d=0, ws_bytes=1 << 20), ARG, "d=0")
        refused(call(lib, d=-1, ws_bytes=1 << 20), ARG, "d=-1")
        refused(call(lib, d=192, ld=188), ARG, "ld=188")
        refused(call(lib, rows=0x1004), ARG, "16-byte aligned")
        refused(call(lib, rows=0x1008), ARG, "16-byte aligned")
        refused(call(lib, d=190, ld=190), ARG, "ld=190")
        refused(call(lib, d=7, ld=9), ARG, "ld=9")
        refused(call(lib, d=1025, ld=1028, ws_bytes=1 << 30), UNSUP, "d=1025")
        refused(call(lib, ws=0x5004), ARG, "aligned")
        assert who in N.last_error()
    refused(_core(lib, k=17, ws_bytes=1 << 30), UNSUP, "k=17")
    refused(_core(lib, k=0, ws_bytes=1 << 30), ARG, "k=0")
    refused(_core(lib, k=-1, ws_bytes=1 << 30), ARG, "k=-1")
    refused(_core(lib, n=10, k=10, ws_bytes=1 << 30), ARG, "k=10")
    refused(_core(lib, n=1, k=1, ws_bytes=1 << 30), ARG, "k=1")
    for call, need in ((_core, int(lib.sd_hdb_core_workspace_bytes(100, 192, 2))), (_outgoing, int(lib.sd_hdb_outgoing_workspace_bytes(100, 192)))):
        assert need > 0
        refused(call(lib, ws_bytes=need - 1), WS, "workspace")
        refused(call(lib, ws_bytes=0), WS, "workspace")


def test_wrappers_and_route_have_no_cpu_fallback():
    from speech_diarization_amd import ops
    hg = _route()
    S = torch.ones(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hdb_core(S, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hdb_outgoing(S, torch.ones(4), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hg.hdbscan_rows(torch.from_numpy(H.planted(40, 2, 0.5, 0, 0)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hg.hdbscan_rows(H.planted(40, 2, 0.5, 0, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hg.DeviceRows("cpu")


# ------------------------------------------------------------------ the driver on the CPU

@pytest.fixture(scope="module")
def rows_of():
    cache = {}

    def get(shape, seed):
        if (shape, seed) not in cache:
            cache[shape, seed] = H.planted(shape[0], shape[1], shape[2], seed, shape[3])
        return cache[shape, seed]
    return get


TREE_CASES = [((300, 4, 0.6, 0), 0, 0), ((300, 4, 0.6, 0), 1, 1), ((700, 3, 0.5, 0), 0, 2), ((1000, 8, 0.8, 20), 1, 4), ((700, 3, 0.5, 0), 2, 16)]


@pytest.mark.parametrize("shape,seed,k", TREE_CASES)
def test_spanning_tree_weights_equal_the_f64_prim_tree(rows_of, shape, seed, k):
    """N - 1 acyclic spanning edges, and the sorted weights are those of an f64 Prim tree of the dense mutual-reachability matrix
    within the f32 dot-product bound (d + 4) 2^-23 |a| |b| of ahc_ref.score_bound (unit rows: 196 x 2^-23).  Every maximum spanning
    tree has the same sorted weights, so this holds under ties; min(., ., .) and sorting are 1-Lipschitz in the max norm, so the bound
    on a product is the bound on a sorted weight."""
    hg = _route()
    X = rows_of(shape, seed)
    n, d = X.shape
    op = H.NumpyRows()
    rows = op.normalise(torch.from_numpy(X))
    core = op.core(rows, k) if k else torch.full((n,), float("inf"))
    info = {"rounds": 0, "gram_rows": 0, "components_per_round": []}
    lo, hi, w = hg.spanning_edges(rows, core, op, info)
    assert H.is_spanning_tree(lo, hi, n)
    assert 1 <= info["rounds"] <= math.ceil(math.log2(n)) and info["components_per_round"][-1] == 1
    assert info["components_per_round"] == sorted(info["components_per_round"], reverse=True)
    core64, W64 = H.reach_f64(rows.numpy(), k)
    bound = float(H.dot_bound(rows.numpy(), d).max())
    assert bound <= (d + 4) * 2.0 ** -23 * 1.001
    if k:
        assert np.abs(core.numpy().astype(np.float64) - core64).max() <= bound
    want = H.prim_max_tree(W64)
    got = np.sort(w.astype(np.float64))[::-1]
    err = float(np.abs(got - want).max())
    print(f"n={n} k={k}: {info['rounds']} rounds {info['components_per_round']}, max |w - w64| {err:.2e}, bound {bound:.2e}")
    assert err <= bound
    # every edge carries the weight of its own pair
    assert np.abs(w.astype(np.float64) - W64[lo, hi]).max() <= bound


def test_spanning_tree_under_massive_ties():
    """Integer rows: a handful of distinct weights, every round full of ties.  The total order keeps the forest acyclic and the sorted
    weights are exactly those of the Prim tree."""
    hg = _route()
    S = H.integer_rows(300, 6, 8, 3, lo=-1, hi=2)[:, :6]
    rows = torch.from_numpy(np.ascontiguousarray(S))
    G = H.gram_f32(S)
    op = H.NumpyRows()
    for k in (0, 1, 3):
        core = torch.from_numpy(H.core_from_gram(G, k).astype(np.float32)) if k else torch.full((300,), float("inf"))
        lo, hi, w = hg.spanning_edges(rows, core, op)
        assert H.is_spanning_tree(lo, hi, 300)
        assert len(np.unique(w)) <= 13
        assert np.array_equal(np.sort(w.astype(np.float64))[::-1], H.prim_max_tree(H.reach_f64(S, k)[1]))


@pytest.mark.parametrize("shape,setting,seed", H.LABEL_CASES)
def test_labels_equal_scikit_learns(rows_of, shape, setting, seed):
    """Same partition and same noise set as sklearn.cluster.HDBSCAN, both for "euclidean" on the rows and for "precomputed" 1 - cos
    against the route's "cosine"."""
    hg = _route()
    X = rows_of(shape, seed)
    op = H.NumpyRows()
    got_e, info = hg.hdbscan_rows(torch.from_numpy(X), *setting, metric="euclidean", operator=op, return_info=True)
    got_c = hg.hdbscan_rows(torch.from_numpy(X), *setting, metric="cosine", operator=op)
    n = X.shape[0]
    passes = 1 if (setting[1] or setting[0]) > 1 else 0
    assert info["gram_rows"] == (info["rounds"] + passes) * n * n and info["rounds"] == len(info["components_per_round"]) <= math.ceil(math.log2(n))
    assert info["mst_weight"] > 0 and got_e.dtype.kind == "i" and got_e.shape == (n,)
    want_e = H.host_labels(X, setting, "euclidean")
    want_c = H.host_labels(X, setting, "precomputed")
    print(f"{shape} {setting} seed {seed}: {info['rounds']} rounds, {len(set(want_e.tolist()) - {-1})} clusters, {int((want_e < 0).sum())} noise")
    assert H.same_clustering(got_e, want_e), "euclidean"
    assert H.same_clustering(got_c, want_c), "cosine against precomputed"


def test_the_recorded_tie_is_a_property_of_the_input():
    """Documents the input, tests no product code (it passes without the route).  In float64, with no kernel and no f32 product involved: at min_samples 3 and 5 the two heaviest edges at row 2 both weigh
    core[2] exactly, and every maximum spanning tree holds two edges of that weight: two sub-trees join through row 2 at one height."""
    (shape, seed) = H.TIED_INPUT
    X = H.unit_rows(H.planted(shape[0], shape[1], shape[2], seed, shape[3]))
    for setting in H.SETTINGS[1:]:
        k = (setting[1] or setting[0]) - 1
        core, W = H.reach_f64(X, k)
        top = np.sort(W[2])[::-1]
        assert top[0] == top[1] == core[2], (setting, top[:3], core[2])
        assert int((H.prim_max_tree(W) == core[2]).sum()) >= 2


def test_label_table_spans_the_settings_and_sizes():
    assert len(H.LABEL_CASES) >= 12 and H.RECORDED_NEAR_TIE not in H.LABEL_CASES
    assert {c[1] for c in H.LABEL_CASES} == set(H.SETTINGS) and {c[0][0] for c in H.LABEL_CASES} == {300, 700, 1000, 2000}
    assert {(c[0][0], c[1]) for c in H.LABEL_CASES} == {(s[0], st) for s in H.SHAPES for st in H.SETTINGS}


@pytest.mark.parametrize("shape,seed", [((1000, 8, 0.8, 20), 0), ((700, 3, 0.5, 0), 1)])
def test_two_stage_glue_equals_the_default_factory(rows_of, shape, seed):
    """Both stages run (micro-clusters, then their centroids); the glue's answer on these inputs is one speaker and 19 / 270 noise rows."""
    hg = _route()
    X = rows_of(shape, seed) * np.float32(3.0)                    # the glue normalises; its centroids come from these rows
    got = cluster.cluster_hdbscan_two_stage(X, 2, clusterer_factory=hg.HdbscanGpuClusterer.factory(operator=H.NumpyRows()))
    want = cluster.cluster_hdbscan_two_stage(X, 2)
    assert H.same_clustering(got, want) and 0 < int((want < 0).sum()) < len(want)


def test_min_samples_one_needs_no_core_pass():
    hg = _route()
    X = H.planted(300, 4, 0.6, 0, 0)
    op = H.NumpyRows()
    got, info = hg.hdbscan_rows(torch.from_numpy(X), 5, 1, True, operator=op, return_info=True)
    assert op.passes == info["rounds"] and info["gram_rows"] == info["rounds"] * 300 * 300
    assert H.same_clustering(got, H.host_labels(X, (5, 1, True), "euclidean"))


def test_clusterer_refuses_precomputed():
    hg = _route()
    with pytest.raises(ValueError, match="precomputed"):
        hg.HdbscanGpuClusterer(2, None, True, "precomputed")
    with pytest.raises(ValueError, match="precomputed"):
        hg.HdbscanGpuClusterer.factory()(min_cluster_size=2, min_samples=None, allow_single_cluster=True, metric="precomputed")
    with pytest.raises(ValueError, match="precomputed"):                                # the single-stage glue hands over a matrix
        cluster.cluster_hdbscan(H.planted(40, 2, 0.5, 0, 0), clusterer_factory=hg.HdbscanGpuClusterer.factory(operator=H.NumpyRows()))
    with pytest.raises(ValueError, match="precomputed"):
        hg.hdbscan_rows(torch.eye(4), metric="precomputed", operator=H.NumpyRows())
    c = hg.HdbscanGpuClusterer.factory(operator=H.NumpyRows())(min_cluster_size=6, min_samples=3, allow_single_cluster=False, metric="euclidean")
    assert (c.min_cluster_size, c.min_samples, c.allow_single_cluster, c.metric) == (6, 3, False, "euclidean")


class Untouchable:
    device = torch.device("cpu")

    def __getattr__(self, name):
        raise AssertionError(f"operator.{name} reached")


def test_bad_arguments_raise_before_the_operator_is_touched():
    hg = _route()
    X = H.planted(40, 2, 0.5, 0, 0)
    with pytest.raises(ValueError, match="min_samples"):
        hg.hdbscan_rows(torch.from_numpy(X), 2, 41, operator=Untouchable())
    with pytest.raises(ValueError, match="min_cluster_size"):
        hg.hdbscan_rows(torch.from_numpy(X), 1, operator=Untouchable())
    for bad in (np.nan, np.inf):
        Xb = X.copy()
        Xb[17, 3] = bad
        for metric in ("euclidean", "cosine"):
            with pytest.raises(ValueError, match="finite"):
                hg.hdbscan_rows(torch.from_numpy(Xb), metric=metric, operator=Untouchable())
    for scale in (0.0, 0.99, 1.01, 3.0):
        Xb = X.copy()
        Xb[5] *= np.float32(scale)
        with pytest.raises(ValueError, match="unit rows"):
            hg.hdbscan_rows(torch.from_numpy(Xb), operator=Untouchable())
    Xb = X.copy()
    Xb[5] *= np.float32(3.0)                                                            # the cosine metric takes any finite rows
    assert H.same_clustering(hg.hdbscan_rows(torch.from_numpy(Xb), metric="cosine", operator=H.NumpyRows()),
                             hg.hdbscan_rows(torch.from_numpy(X), metric="cosine", operator=H.NumpyRows()))


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_inputs(n):
    hg = _route()
    X = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0]], np.float32)[:n]
    got, info = hg.hdbscan_rows(torch.from_numpy(X), operator=Untouchable() if n < 2 else H.NumpyRows(), return_info=True)
    assert got.tolist() == [0] * n and got.dtype.kind == "i"
    if n == 2:
        assert H.same_clustering(got, H.host_labels(X, (2, None, True), "euclidean")) and info["rounds"] == 1


def test_a_missing_private_function_names_the_version(monkeypatch):
    hg = _route()
    import sklearn.cluster._hdbscan.hdbscan as private
    monkeypatch.delattr(private, "_process_mst")
    with pytest.raises(ImportError, match=r"scikit-learn 1\.7\.2"):
        hg.hdbscan_rows(torch.from_numpy(H.planted(40, 2, 0.5, 0, 0)), operator=H.NumpyRows())


# ------------------------------------------------------------------ the public interface

def _fft_encoder(w):
    return np.stack([np.abs(np.fft.rfft(r, 382))[:192] for r in np.asarray(w, dtype=np.float32)]).astype(np.float32)


def test_diarize_reaches_the_device_clusterer(monkeypatch):
    """`diarize(clusterer="hdbscan_gpu")` runs the two-stage glue over `HdbscanGpuClusterer.factory()`: with the factory patched to the
    numpy operator it gives the default clusterer's segments, and the clusterer was built with the glue's four keywords."""
    hg = _route()
    from speech_diarization_amd import anti_stick_diarize as asd
    from speech_diarization_amd import synth
    y = synth.synthetic_conversation(20.0, 2, seed=0).wav

    def vad(y, sr, **kw):
        return [(0.5 * i, 0.5 * i + 0.45) for i in range(int(len(y) / sr / 0.5))]
    seen = []

    product_factory = hg.HdbscanGpuClusterer.factory

    def factory(operator=None):
        assert operator is None
        inner = product_factory(operator=H.NumpyRows())

        def make(**kw):
            seen.append(kw)
            return inner(**kw)
        return make
    want = asd.diarize(y, encode=_fft_encoder, vad_segments=vad, scd_thr=1e9, reseg=0)
    monkeypatch.setattr(hg.HdbscanGpuClusterer, "factory", staticmethod(factory))
    got = asd.diarize(y, encode=_fft_encoder, vad_segments=vad, scd_thr=1e9, reseg=0, clusterer="hdbscan_gpu")
    assert seen and all(kw == dict(min_cluster_size=2, min_samples=None, metric="euclidean", allow_single_cluster=True) for kw in seen)
    assert [(s.start, s.end, s.spk) for s in got] == [(s.start, s.end, s.spk) for s in want] and len(got) >= 1
    with pytest.raises(ValueError, match="'hdbscan_gpu'"):
        asd.diarize(y, encode=_fft_encoder, vad_segments=vad, clusterer="no such clusterer")


def test_cluster_hdbscan_rows_route_argument_rules():
    from speech_diarization_amd import anti_stick_diarize as asd
    X = H.planted(40, 2, 0.5, 0, 0)
    assert asd.cluster_hdbscan(X[:1], use_gpu="rows").tolist() == [0]
    with pytest.raises(ValueError, match="use_gpu"):
        asd.cluster_hdbscan(X, use_gpu="columns")
    with pytest.raises(ValueError, match="clusterer_factory"):
        asd.cluster_hdbscan(X, clusterer_factory=cluster.default_hdbscan_factory, use_gpu="rows")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            asd.cluster_hdbscan(X, use_gpu="rows")
