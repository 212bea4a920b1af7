"""No-GPU checks of the device AHC route (include/sd_hip_ahc.h, speech-diarization_amd/ahc_gpu.py): the binding table, the workspace
formula, the refusals an entry makes before it launches anything, and the driver itself run on the CPU through an injected numpy
operator against `cluster.ahc_cosine`."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import ahc_ref as A  # noqa: E402
from abi_rules import ARG, UNSUP, WS, check_header_and_table, check_versions, refused  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import ahc_gpu, cluster  # noqa: E402


# ------------------------------------------------------------------ ABI

def test_header_and_binding_table_name_the_same_exported_entries():
    check_header_and_table("sd_hip_ahc.h", N.AHC_PROTOTYPES, (N.PROTOTYPES, N.SPECTRAL_PROTOTYPES))


def test_versions():
    assert N.SD_AHC_ABI_VERSION == 1
    check_versions(sd_ahc_abi_version=1, sd_abi_version=11, sd_spectral_abi_version=1)      # the main ABI and the spectral one are untouched


def test_workspace_formula():
    """(T + 1) slots of 128 T padded rows, a score and an index each; d does not enter beyond its range."""
    lib = N.load()
    for n in (1, 5, 127, 128, 129, 257, 1000, 7609, 50000):
        t = -(-n // 128)
        for d in (1, 7, 190, 192, 1024):
            assert int(lib.sd_ahc_nearest_workspace_bytes(n, d)) == (t + 1) * t * 128 * 8, (n, d)
    assert int(lib.sd_ahc_nearest_workspace_bytes(128, 192)) == 2048 and int(lib.sd_ahc_nearest_workspace_bytes(129, 192)) == 6144
    for n, d in ((0, 192), (-3, 192), (100, 0), (100, -1), (100, 1025)):
        assert int(lib.sd_ahc_nearest_workspace_bytes(n, d)) == 0, (n, d)


# ------------------------------------------------------------------ refusals before launch (no device needed: fake non-null pointers)

def _nearest(lib, sums=0x1000, ld=192, n=100, d=192, inv_count=0x2000, nn=0x3000, best=0x4000, ws=0x5000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = int(lib.sd_ahc_nearest_workspace_bytes(n, d)) if n > 0 else 0
    return lib.sd_ahc_nearest_f32(sums, ld, n, d, inv_count, nn, best, ws, ws_bytes, None)


def _merge(lib, sums=0x1000, ld=192, n=100, d=192, count=0x2000, inv_count=0x3000, nn=0x4000, best=0x5000, cos_thr=0.7, target=0x6000,
           n_merged=0x7000):
    return lib.sd_ahc_merge_f32(sums, ld, n, d, count, inv_count, nn, best, cos_thr, target, n_merged, None)


def test_refusals_happen_before_anything_is_launched():
    """Every case returns its own argument / support / workspace code with a message.  A launch on this pointer soup would have
    returned SD_ERR_HIP (no device here) or faulted (on a GPU)."""
    lib = N.load()
    for name in ("sums", "inv_count", "nn", "best", "ws"):
        refused(_nearest(lib, **{name: None}), ARG, "null pointer")
    for name in ("sums", "count", "inv_count", "nn", "best", "target", "n_merged"):
        refused(_merge(lib, **{name: None}), ARG, "null pointer")
    for call, who in ((_nearest, "sd_ahc_nearest_f32"), (_merge, "sd_ahc_merge_f32")):
        refused(call(lib, n=0), ARG, "n=0")
        refused(call(lib, n=-5), ARG, "n=-5")
        refused(call(lib, d=0), ARG, "d=0")
        refused(call(lib, d=-1), ARG, "d=-1")
        refused(call(lib, d=192, ld=188), ARG, "ld=188")
        refused(call(lib, sums=0x1004), ARG, "16-byte aligned")
        refused(call(lib, sums=0x1008), ARG, "16-byte aligned")
        refused(call(lib, d=190, ld=190), ARG, "ld=190")
        refused(call(lib, d=7, ld=9), ARG, "ld=9")
        assert who in N.last_error()
    refused(_nearest(lib, d=1025, ld=1028, ws_bytes=1 << 30), UNSUP, "d=1025")
    refused(_nearest(lib, ws=0x5004), ARG, "aligned")
    need = int(lib.sd_ahc_nearest_workspace_bytes(100, 192))
    refused(_nearest(lib, ws_bytes=need - 1), WS, "workspace")
    refused(_nearest(lib, ws_bytes=0), WS, "workspace")


def test_wrappers_and_route_have_no_cpu_fallback():
    from speech_diarization_amd import ops
    S = torch.ones(4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ahc_nearest(S, torch.ones(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ahc_merge(S, torch.ones(4), torch.ones(4), torch.zeros(4, dtype=torch.int32), torch.ones(4), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahc_gpu.ahc_cosine_rows(torch.ones(40, 8), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahc_gpu.ahc_cosine_rows(np.ones((40, 8), np.float32), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ahc_gpu.DeviceSums("cpu")


def test_pipeline_refuses_ahc_gpu_with_an_injected_encoder():
    from speech_diarization_amd import diarization_baseline as db
    from speech_diarization_amd import synth
    y = synth.synthetic_conversation(12.0, 2, seed=0).wav

    def enc(w):
        return np.stack([np.abs(np.fft.rfft(r, 382))[:192] for r in np.asarray(w, dtype=np.float32)]).astype(np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        db.diarize_audio({"waveform": y, "sample_rate": 16000}, 0.35, 0.1, 2, 6, encoder=enc, clustering="ahc_gpu")


# ------------------------------------------------------------------ the driver on the CPU

def _same_partition(got, want):
    return np.array_equal(cluster.relabel_by_first_appearance(got), cluster.relabel_by_first_appearance(want))


@pytest.fixture(scope="module")
def affinities():
    cache = {}

    def get(rows):
        if rows not in cache:
            X, _ = A.family_rows(rows)
            cache[rows] = (X, A.host_affinity(X))
        return cache[rows]
    return get


@pytest.mark.parametrize("rows,thr", A.DRIVER_PAIRS)
def test_partition_equals_the_host_route(affinities, rows, thr):
    """Condition on the input first: the host dendrogram has no merge height within 1e-3 of the cut (a near-tie tests luck)."""
    X, K = affinities(rows)
    margin = A.cut_margin(K, thr)
    assert margin > A.CUT_MARGIN, margin
    want = cluster.ahc_cosine(K, thr)
    op = A.NumpySums()
    got, info = ahc_gpu.ahc_cosine_rows(torch.from_numpy(X), thr, operator=op, return_info=True)
    print(f"rows={rows} thr={thr}: cut margin {margin:.2e}, {info['clusters']} clusters, {info['rounds']} rounds, "
          f"gram_rows / N^2 {info['gram_rows'] / rows ** 2:.2f}, last_best {info['last_best']:.4f}")
    assert _same_partition(got, want), f"{int((got != cluster.relabel_by_first_appearance(want)).sum())} of {rows} labels differ"
    assert np.array_equal(got, cluster.relabel_by_first_appearance(got))                # numbered by first appearance
    assert info["clusters"] == len(np.unique(want)) and op.passes == info["rounds"] + 1
    assert info["last_best"] <= thr or info["clusters"] == 1
    assert info["gram_rows"] >= rows * rows


@pytest.mark.parametrize("thr", [0.3, 0.05])
def test_duplicate_rows_and_zero_rows(thr):
    """Duplicates score exactly 1 with each other and tie everywhere else; a zero row has similarity 0 to everything, as sklearn's
    cosine_similarity gives."""
    X = A.duplicates_and_zero_rows()
    K = A.host_affinity(X)
    assert np.all(K[-3:] == 0)
    want = cluster.ahc_cosine(K, thr)
    got = ahc_gpu.ahc_cosine_rows(torch.from_numpy(X), thr, operator=A.NumpySums())
    assert _same_partition(got, want)
    assert np.array_equal(got[300:350], got[:50])                                       # a duplicate sits with its original


def test_nan_row_raises_before_the_operator_is_touched():
    class Untouchable:
        device = torch.device("cpu")

        def __getattr__(self, name):
            raise AssertionError(f"operator.{name} reached")
    X, _ = A.family_rows(400)
    for bad in (np.nan, np.inf):
        Xb = X.copy()
        Xb[17, 3] = bad
        with pytest.raises(ValueError, match="finite"):
            ahc_gpu.ahc_cosine_rows(torch.from_numpy(Xb), 0.3, operator=Untouchable())


@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_inputs_take_the_host_functions_returns(n):
    X = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0]], np.float32)[:n]
    K = A.host_affinity(X) if n else np.zeros((0, 0), np.float32)
    for thr in (0.5, 0.7):                                                              # the two rows have cosine 0.6
        got, info = ahc_gpu.ahc_cosine_rows(torch.from_numpy(X), thr, operator=A.NumpySums(), return_info=True)
        assert np.array_equal(got, cluster.relabel_by_first_appearance(cluster.ahc_cosine(K, thr))), (n, thr)
        assert info["clusters"] == len(set(got.tolist())) and got.dtype.kind == "i"


def test_threshold_above_every_score_leaves_singletons_in_no_round():
    X, _ = A.family_rows(400)
    op = A.NumpySums()
    got, info = ahc_gpu.ahc_cosine_rows(torch.from_numpy(X), 1.5, operator=op, return_info=True)
    assert np.array_equal(got, np.arange(400))
    assert info["rounds"] == 0 and info["clusters"] == 400 and info["gram_rows"] == 400 * 400 and op.passes == 1
    assert info["last_best"] < 1.5


def test_clusterer_refuses_precomputed_and_matches_the_host_clusterer_on_rows():
    with pytest.raises(ValueError, match="precomputed"):
        ahc_gpu.AhcGpuClusterer(0.3, metric="precomputed")
    with pytest.raises(ValueError, match="precomputed"):
        ahc_gpu.AhcGpuClusterer.factory(0.3)(min_cluster_size=2, metric="precomputed")
    with pytest.raises(ValueError, match="precomputed"):                                # the single-stage glue hands over a matrix
        cluster.cluster_hdbscan(A.family_rows(400)[0], clusterer_factory=ahc_gpu.AhcGpuClusterer.factory(0.3))
    X, _ = A.family_rows(400)
    got = cluster.cluster_hdbscan_two_stage(X, clusterer_factory=ahc_gpu.AhcGpuClusterer.factory(0.3, operator=A.NumpySums()))
    want = cluster.cluster_hdbscan_two_stage(X, clusterer_factory=cluster.AhcClusterer.factory(0.3))
    assert _same_partition(got, want) and len(set(got.tolist())) >= 2
