"""No-GPU checks of the device spectral route (include/sd_hip_spectral.h, speech-diarization_amd/cluster_gpu.py): the binding table, the
workspace formula, the refusals an entry makes before it launches anything, and the solver itself run on the CPU through an injected numpy
operator against `np.linalg.eigvalsh`, `cluster.estimate_num_speakers` and `cluster.spectral`."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import spectral_ref as R  # noqa: E402
from abi_rules import ARG, UNSUP, WS, check_header_and_table, check_versions, refused  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import cluster, cluster_gpu  # noqa: E402

warnings.filterwarnings("ignore", message="Graph is not fully connected")

# Eigenvalue bar of the solver against f64 eigvalsh.  The operator is f32: S V carries a relative rounding error of about 2^-24 per
# product and sum, random in sign, so a Rayleigh quotient u^T (S + E) u of a unit vector moves by about ||E|| <= 2^-24 sqrt(log N)
# ~ 2e-7 at worst and far less on average; the iteration adds residual^2 / gap <= (1e-5)^2 / 1e-3.  1e-7 covers both.
EIG_BAR = 1e-7

# (N, planted speakers, noise, seed): centred planted-cluster rows, N 400 .. 2000, k 2 .. 8, noise 0.9 .. 3.0
FAMILIES = [(400, 2, 0.9, 0), (700, 3, 1.5, 0), (1000, 4, 2.0, 0), (1300, 5, 2.5, 1), (1600, 6, 3.0, 0), (2000, 8, 1.2, 0)]
MIN_SPK, MAX_SPK = 1, 12


# ------------------------------------------------------------------ ABI

def test_header_and_binding_table_name_the_same_exported_entries():
    check_header_and_table("sd_hip_spectral.h", N.SPECTRAL_PROTOTYPES, (N.PROTOTYPES,))


def test_versions():
    assert N.SD_SPECTRAL_ABI_VERSION == 1
    check_versions(sd_spectral_abi_version=1, sd_abi_version=11)      # the main ABI is untouched by the new header


def _splits(n):
    chunks = -(-n // 256)
    want = min(chunks, max(1, 2048 // -(-n // 128)))
    per = max(min(2, chunks), -(-chunks // want))
    return -(-chunks // per)


def test_workspace_formula():
    lib = N.load()
    for n in (1, 5, 127, 128, 129, 255, 256, 257, 1000, 3001, 7609, 20000, 50000, 131072):
        for b in (8, 16, 24, 32):
            want = (_splits(n) * n * b * 4 + 255) // 256 * 256
            assert int(lib.sd_affinity_apply_workspace_bytes(n, b)) == want, (n, b)
    assert _splits(7609) == 15 and _splits(50000) == 5 and _splits(100) == 1 and _splits(257) == 1 and _splits(513) == 2
    for n, b in ((0, 16), (-3, 16), (100, 0), (100, 12), (100, 40), (100, -8)):
        assert int(lib.sd_affinity_apply_workspace_bytes(n, b)) == 0, (n, b)


# ------------------------------------------------------------------ refusals before launch (no device needed: fake non-null pointers)

def _apply(lib, K=0x1000, n=100, ld=100, zd=0, scale=0x2000, V=0x3000, ldv=16, b=16, Y=0x4000, ldy=16, ws=0x5000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = int(lib.sd_affinity_apply_workspace_bytes(n, b)) if n > 0 else 0
    return lib.sd_affinity_apply_f32(K, n, ld, zd, scale, V, ldv, b, Y, ldy, ws, ws_bytes, None)


def test_refusals_happen_before_anything_is_launched():
    """Every case returns its own argument / support / workspace code with a message.  A launch on this pointer soup would have
    returned SD_ERR_HIP (no device here) or faulted (on a GPU)."""
    lib = N.load()
    refused(lib.sd_affinity_degree_f32(None, 10, 10, 0, 0x1000, None), ARG, "null pointer")
    refused(lib.sd_affinity_degree_f32(0x1000, 10, 10, 0, None, None), ARG, "null pointer")
    refused(lib.sd_affinity_degree_f32(0x1000, 0, 10, 0, 0x2000, None), ARG, "N=0")
    refused(lib.sd_affinity_degree_f32(0x1000, -1, 10, 0, 0x2000, None), ARG, "N=-1")
    refused(lib.sd_affinity_degree_f32(0x1000, 10, 9, 1, 0x2000, None), ARG, "ld=9")
    for name in ("K", "scale", "V", "Y", "ws"):
        refused(_apply(lib, **{name: None}), ARG, "null pointer")
    for b in (0, 4, 12, 20, 33, 40, 64, -8):
        refused(_apply(lib, b=b, ldv=64, ldy=64, ws_bytes=1 << 30), UNSUP, f"b={b}")
    refused(_apply(lib, n=0), ARG, "N=0")
    refused(_apply(lib, n=-5), ARG, "N=-5")
    refused(_apply(lib, n=100, ld=99), ARG, "ld=99")
    refused(_apply(lib, b=24, ldv=23, ldy=24), ARG, "ldv=23")
    refused(_apply(lib, b=24, ldv=24, ldy=16), ARG, "ldy=16")
    refused(_apply(lib, ws=0x5004), ARG, "aligned")
    need = int(lib.sd_affinity_apply_workspace_bytes(100, 16))
    refused(_apply(lib, ws_bytes=need - 1), WS, "workspace")
    refused(_apply(lib, ws_bytes=0), WS, "workspace")


def test_wrappers_and_route_have_no_cpu_fallback():
    from speech_diarization_amd import ops
    K = torch.eye(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.affinity_degree(K)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.affinity_apply(K, torch.ones(4), torch.ones(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster_gpu.estimate_num_speakers(torch.eye(40), 2, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cluster_gpu.spectral(torch.eye(40), 3)


def test_pipeline_refuses_spectral_gpu_with_an_injected_encoder():
    from speech_diarization_amd import diarization_baseline as db
    from speech_diarization_amd import synth
    y = synth.synthetic_conversation(12.0, 2, seed=0).wav

    def enc(w):
        return np.stack([np.abs(np.fft.rfft(r, 382))[:192] for r in np.asarray(w, dtype=np.float32)]).astype(np.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        db.diarize_audio({"waveform": y, "sample_rate": 16000}, 0.35, 0.1, 2, 6, encoder=enc, clustering="spectral_gpu")
    with pytest.raises(ValueError, match="unknown clustering"):
        db.diarize_audio({"waveform": y, "sample_rate": 16000}, 0.35, 0.1, 2, 6, encoder=enc, clustering="spectral_tpu")


# ------------------------------------------------------------------ the solver on the CPU

@pytest.mark.parametrize("n", [300, 1000, 3000])
def test_top_eigenpairs_against_eigvalsh(n):
    """Numpy f32 operator, small algebra in f64: the 13 leading eigenvalues of S against f64 eigvalsh of the same (f32-rounded) matrix,
    the eigenvectors through their residual in f64."""
    X, _ = R.planted_rows(n, 5, 1.5, seed=n)
    A = np.clip(R.cosine(X), 0.0, None).astype(np.float32)
    d = A.sum(1, dtype=np.float64)
    s = (1.0 / np.sqrt(d)).astype(np.float32)
    S32 = (s[:, None] * A * s[None, :]).astype(np.float32)
    S64 = S32.astype(np.float64)
    passes = []

    def apply(V):
        passes.append(V.shape[1])
        return S32 @ V.numpy()
    theta, U, info = cluster_gpu.top_eigenpairs(apply, n, 13, block=24, tol=1e-5, max_steps=40, seed=0)
    ref = np.sort(np.linalg.eigvalsh(S64))[::-1][:13]
    print(f"n={n}: passes {info['passes']}, residual {info['residual']:.2e}, max eigenvalue error {np.abs(theta - ref).max():.2e}")
    assert info["passes"] == len(passes) <= 20 and info["residual"] <= 1e-5
    assert np.abs(theta - ref).max() <= EIG_BAR
    U = U.numpy()
    assert np.abs(U.T @ U - np.eye(13)).max() <= 1e-10
    assert np.linalg.norm(S64 @ U - U * theta, axis=0).max() <= 2e-5
    # deterministic: the start block is seeded and drawn on the host
    theta2, U2, _ = cluster_gpu.top_eigenpairs(lambda V: S32 @ V.numpy(), n, 13, seed=0)
    assert np.array_equal(theta, theta2) and np.array_equal(U, U2.numpy())


def test_top_eigenpairs_survives_a_converged_basis():
    """A rank-3 operator: after the second pass the new block has no direction left.  The iteration must stop there (or run on without
    breaking down when told to continue to 40 passes with an unreachable tolerance) and return the exact pairs."""
    rng = np.random.default_rng(3)
    B = np.linalg.qr(rng.standard_normal((500, 3)))[0]
    S = (B * np.array([0.9, 0.5, 0.2])) @ B.T
    S32 = S.astype(np.float32)
    for tol in (1e-5, 0.0):
        theta, U, info = cluster_gpu.top_eigenpairs(lambda V: S32 @ V.numpy(), 500, 5, block=8, tol=tol, max_steps=40, seed=1)
        assert info["passes"] <= 40 and np.all(np.isfinite(theta)) and bool(torch.isfinite(U).all())
        assert np.abs(theta - np.array([0.9, 0.5, 0.2, 0.0, 0.0])).max() <= EIG_BAR, theta


@pytest.mark.parametrize("n,k,noise,seed", FAMILIES)
def test_count_and_partition_equal_the_host_functions(n, k, noise, seed):
    X, planted = R.planted_rows(n, k, noise, seed)
    K = R.cosine(X).astype(np.float32)
    # condition on the input: the host's deciding eigengap leads its runner-up by at least 100 eigenvalue bars (a near-tie tests luck)
    ev, gaps = R.host_eigengaps(K, MIN_SPK, MAX_SPK)
    top2 = np.sort(gaps)[::-1][:2]
    print(f"n={n} k={k} noise={noise}: deciding gap {top2[0]:.4f}, runner-up {top2[1]:.4f} (ratio {top2[0] / top2[1]:.2f})")
    assert top2[0] - top2[1] >= 100 * EIG_BAR
    want_k = cluster.estimate_num_speakers(K, MIN_SPK, MAX_SPK)
    op = R.NumpyOperator(K)
    got_k, info = cluster_gpu.estimate_num_speakers(None, MIN_SPK, MAX_SPK, operator=op, return_info=True)
    assert np.abs(info["eigenvalues"] - ev).max() <= EIG_BAR
    assert got_k == want_k
    assert op.passes == info["passes"] <= 20
    kk = max(want_k, k)                                   # the planted count where the eigengap says 1: there is nothing to partition at 1
    want = cluster.relabel_by_first_appearance(cluster.spectral(K, kk))
    got = cluster.relabel_by_first_appearance(cluster_gpu.spectral(None, kk, operator=R.NumpyOperator(K)))
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {n} labels differ"
    assert len(np.unique(got)) == kk


# ------------------------------------------------------------------ edge cases

@pytest.mark.parametrize("n", [0, 1, 2])
def test_tiny_inputs_take_the_host_functions_returns(n):
    K = np.ones((n, n), np.float32)
    for lo, hi in ((1, 8), (2, 8), (2, 2), (3, 1)):
        assert cluster_gpu.estimate_num_speakers(None, lo, hi, operator=R.NumpyOperator(K)) == cluster.estimate_num_speakers(K, lo, hi), (n, lo, hi)
    for ks in (0, 1, 2, 3):
        assert np.array_equal(cluster_gpu.spectral(None, ks, operator=R.NumpyOperator(K)), cluster.spectral(K, ks)), (n, ks)


def test_n_speakers_at_least_n():
    X, _ = R.planted_rows(6, 2, 0.9, 0)
    K = R.cosine(X).astype(np.float32)
    for ks in (6, 7, 100):
        got = cluster_gpu.spectral(None, ks, operator=R.NumpyOperator(K))
        assert np.array_equal(got, np.arange(6)) and np.array_equal(got, cluster.spectral(K, ks))
    # n just above n_speakers: the Krylov space is the whole space
    got = cluster.relabel_by_first_appearance(cluster_gpu.spectral(None, 2, operator=R.NumpyOperator(K)))
    assert np.array_equal(got, cluster.relabel_by_first_appearance(cluster.spectral(K, 2)))


def test_zero_degree_row():
    """A row with no positive affinity (its own diagonal included) has degree 0 and scale 1 in both functions."""
    X, _ = R.planted_rows(300, 3, 1.0, 5)
    K = R.cosine(X).astype(np.float32)
    K[17, :] = -0.25
    K[:, 17] = -0.25
    want_k = cluster.estimate_num_speakers(K, 2, 8)
    got_k, info = cluster_gpu.estimate_num_speakers(None, 2, 8, operator=R.NumpyOperator(K), return_info=True)
    ev, _ = R.host_eigengaps(K, 2, 8)
    assert np.all(np.isfinite(info["eigenvalues"])) and np.abs(info["eigenvalues"] - ev).max() <= EIG_BAR
    assert got_k == want_k
    op = R.NumpyOperator(K)
    assert float(op.degree(True)[17]) == 0.0
    emb, _ = cluster_gpu.spectral_embedding(None, 3, operator=op)
    assert np.all(np.isfinite(emb))
    got = cluster.relabel_by_first_appearance(cluster_gpu.spectral(None, 3, operator=R.NumpyOperator(K)))
    want = cluster.relabel_by_first_appearance(cluster.spectral(K, 3))
    keep = np.arange(300) != 17                           # the isolated row's embedding is 0 in every component: its label is k-means' tie
    assert np.array_equal(cluster.relabel_by_first_appearance(got[keep]), cluster.relabel_by_first_appearance(want[keep]))


def test_disconnected_graph():
    """Three components: eigenvalue 0 of the Laplacian three times.  The eigenvectors of a repeated eigenvalue are not unique, so the
    check is on what is: the count, the eigenvalues, and a partition equal to the components (which the host route finds too)."""
    sizes = (40, 70, 50)
    comp = np.repeat(np.arange(3), sizes)
    rng = np.random.default_rng(11)
    K = np.where(comp[:, None] == comp[None, :], rng.uniform(0.3, 0.9, (160, 160)), -0.2)
    K = (0.5 * (K + K.T)).astype(np.float32)
    np.fill_diagonal(K, 1.0)
    got_k, info = cluster_gpu.estimate_num_speakers(None, 1, 8, operator=R.NumpyOperator(K), return_info=True)
    assert got_k == 3 == cluster.estimate_num_speakers(K, 1, 8)
    assert np.abs(info["eigenvalues"][:3]).max() <= EIG_BAR
    got = cluster.relabel_by_first_appearance(cluster_gpu.spectral(None, 3, operator=R.NumpyOperator(K)))
    assert np.array_equal(got, comp)
    assert np.array_equal(cluster.relabel_by_first_appearance(cluster.spectral(K, 3)), comp)
