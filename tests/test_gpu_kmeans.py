"""The device k-means on the MI355X (include/sd_hip_kmeans.h: sd_kmeans_grouped_f64; kmeans_gpu.py; cluster_gpu.spectral with
assign_labels="device"; clustering="spectral_device"): scikit-learn's labels, integer for integer, for recordings of every critical size
in one launch, the parameter variants, guard bands at exact buffer sizes, every flag, and the public routes.  Every launch runs
under the launch log, held to its two kernels, and twice with identical bytes."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import guarded as G  # noqa: E402
import kmeans_ref as KR  # noqa: E402
import spectral_ref as R  # noqa: E402
from launch_log import expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu

KERNELS = {"kmeans_lloyd_kernel", "kmeans_select_kernel"}


@pytest.fixture(scope="module")
def dev():
    from speech_diarization_amd import _native as N
    N.load()
    return torch.device("cuda")


def _launch(dev, recs, ks, draws, *, n_init=10, max_iter=300, tol=1e-4, pad=3, first_row=None, max_k=None, max_rows=None, poison=0xFF):
    """One call of the entry on guarded buffers of exactly the sizes the header names: the rows with ld = dim + pad (the last row ends
    after dim columns), the tables, the five outputs, the workspace -> (labels, chosen, inertia, iters, flags) as numpy.  `draws`:
    [(first [n_init], u [n_init, 31, 5])] per recording."""
    from speech_diarization_amd import _native as N
    from speech_diarization_amd import ops
    import ctypes as C
    sizes = [len(x) for x in recs]
    n, dim, ng = sum(sizes), recs[0].shape[1], len(recs)
    ld = dim + pad
    flat = np.full(max(n * ld - pad, 0), np.nan)
    X = np.concatenate(recs)
    for j in range(dim):
        flat[j::ld] = X[:, j]
    fr = np.concatenate([[0], np.cumsum(sizes)]) if first_row is None else np.asarray(first_row)
    rows = G.guarded_from(torch.from_numpy(flat), dev, "rows")
    t_fr = G.guarded_from(torch.from_numpy(fr.astype(np.int32)), dev, "first_row")
    t_k = G.guarded_from(torch.from_numpy(np.asarray(ks, np.int32)), dev, "k")
    t_first = G.guarded_from(torch.from_numpy(np.stack([f for f, _ in draws]).astype(np.int32)), dev, "first")
    t_u = G.guarded_from(torch.from_numpy(np.stack([u for _, u in draws]).astype(np.float64)), dev, "u")
    labels = G.guarded(4 * n, poison, dev, "labels")
    chosen, iters, flags = (G.guarded(4 * ng, poison, dev, name) for name in ("chosen", "iters", "flags"))
    inertia = G.guarded(8 * ng, poison, dev, "inertia")
    need = int(N.load().sd_kmeans_grouped_workspace_bytes(n, ng, n_init))
    assert need == 12 * n_init * n + 16 * n_init * ng
    ws = G.guarded(need, poison, dev, "ws")
    bufs = (rows, t_fr, t_k, t_first, t_u, labels, chosen, iters, flags, inertia, ws)
    with expect_launches(exactly=KERNELS) as log:
        ops.launch("sd_kmeans_grouped_f64", ws.raw, rows.ptr, ld, n, dim, t_fr.ptr, ng, t_k.ptr, n_init, max_iter, C.c_double(tol),
                   max(ks) if max_k is None else max_k, max(sizes) if max_rows is None else max_rows, t_first.ptr, t_u.ptr, labels.ptr, chosen.ptr,
                   inertia.ptr, iters.ptr, flags.ptr, ws.ptr, need)
        torch.cuda.synchronize()
    assert log == {k: 1 for k in KERNELS}
    G.assert_guards_intact(*bufs)
    assert np.array_equal(rows.view(torch.float64).cpu().numpy(), flat, equal_nan=True)            # the inputs are only read
    return tuple(b.view(dt).cpu().numpy().copy() for b, dt in ((labels, torch.int32), (chosen, torch.int32), (inertia, torch.float64),
                                                              (iters, torch.int32), (flags, torch.int32)))


def _twice(dev, recs, ks, draws, **kw):
    """Two launches, a different poison under the outputs each time: identical bytes"""
    a = _launch(dev, recs, ks, draws, poison=G.POISONS[0], **kw)
    b = _launch(dev, recs, ks, draws, poison=G.POISONS[1], **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    return a


def _draws(cases, n_init=10):
    return [KR.draws_padded(np.random.RandomState(seed), len(X), k, n_init) for X, k, seed in cases]


def _check(out, cases, want, order=None):
    labels, chosen, inertia, iters, flags = out
    order = range(len(cases)) if order is None else order
    at = 0
    for slot, g in enumerate(order):
        X, k, seed = cases[g]
        got = labels[at:at + len(X)]
        at += len(X)
        assert flags[slot] == 0, (g, flags[slot])
        assert got.dtype == np.int32 and np.array_equal(got, want[g][0]), f"recording {g} ({X.shape}, k={k}): {int((got != want[g][0]).sum())} labels differ"
        assert iters[slot] == want[g][2] and abs(inertia[slot] - want[g][1]) <= 1e-9 * want[g][1] and 0 <= chosen[slot] < 16


_REFERENCE = {}


def _reference(key, cases, **kw):
    """scikit-learn's answers, computed once per set of cases and shared; the margin condition on the inputs is checked with them"""
    if key not in _REFERENCE:
        want, trace, flags = KR.reference(cases, **kw)
        assert not any(flags) and all(v >= KR.MARGIN_BAR for v in trace.margins.values()), (flags, trace.margins)
        _REFERENCE[key] = want
    return _REFERENCE[key]


@pytest.mark.parametrize("d", KR.GPU_DIMS)
def test_every_critical_size_in_one_launch_equals_scikit_learn(dev, d):
    """n in {3, 63, 64, 65, 255, 256, 257, 1000} and a recording whose rows cannot live in LDS, in two orders"""
    cases = KR.gpu_cases(d)
    want = _reference(("sizes", d), cases)
    draws = _draws(cases)
    for order in (list(range(len(cases))), list(range(len(cases)))[::-1]):
        out = _twice(dev, [cases[g][0] for g in order], [cases[g][1] for g in order], [draws[g] for g in order])
        _check(out, cases, want, order)
    # the bits do not depend on where the rows were read from: everything streamed (max_rows = 1) gives the same bytes
    streamed = _launch(dev, [c[0] for c in cases], [c[1] for c in cases], draws, max_rows=1)
    lds = _launch(dev, [c[0] for c in cases], [c[1] for c in cases], draws)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(streamed, lds))


def test_the_blob_cases_in_one_launch(dev):
    """The twelve cases of the rule tests in one launch: a launch has one column count, so their columns are padded to 32 with zeros.
    A zero column changes no distance, but it lowers the mean column variance and with it the tolerance: scikit-learn gets the
    padded rows too."""
    cases = [(np.pad(KR.blob(*c), ((0, 0), (0, 32 - c[1]))), c[2], c[4]) for c in KR.BLOBS]
    want = _reference("blobs", cases)
    _check(_twice(dev, [c[0] for c in cases], [c[1] for c in cases], _draws(cases)), cases, want)


@pytest.mark.parametrize("kw", [{"n_init": 1}, {"n_init": 3}, {"n_init": 10}, {"max_iter": 3}, {"tol": 0}], ids=str)
def test_parameter_variants(dev, kw):
    cases = KR.gpu_cases(8)
    want = _reference(("variant", str(kw)), cases, **kw)
    n_init = kw.get("n_init", 10)
    out = _twice(dev, [c[0] for c in cases], [c[1] for c in cases], _draws(cases, n_init), n_init=n_init, max_iter=kw.get("max_iter", 300),
                 tol=kw.get("tol", 1e-4))
    _check(out, cases, want)
    if "max_iter" in kw:
        assert out[3].max() == 3


def test_every_flag(dev):
    good = KR.gpu_cases(2)[1:5]
    want = _reference("flags", good)
    draws = _draws(good)
    deg = KR.degenerate_rows()
    # EMPTY: fewer distinct rows than clusters; its neighbours are unaffected
    recs, ks = [good[0][0], deg, good[1][0]], [good[0][1], 5, good[1][1]]
    dr = [draws[0], KR.draws_padded(np.random.RandomState(0), 40, 5, 10), draws[1]]
    out = _twice(dev, recs, ks, dr)
    assert out[4].tolist() == [0, KR.EMPTY, 0] and (out[0][63:103] == -1).all() and out[1][1] == -1 and out[2][1] == 0 and out[3][1] == 0
    assert np.array_equal(out[0][:63], want[0][0]) and np.array_equal(out[0][103:], want[1][0])
    # NONFINITE: a NaN, an inf
    for value in (np.nan, np.inf, -np.inf):
        bad = good[2][0].copy()
        bad[len(bad) - 1, 1] = value
        out = _twice(dev, [good[0][0], bad, good[3][0]], [good[0][1], good[2][1], good[3][1]], [draws[0], draws[2], draws[3]])
        assert out[4].tolist() == [0, KR.NONFINITE, 0] and (out[0][63:63 + 65] == -1).all(), value
        assert np.array_equal(out[0][:63], want[0][0]) and np.array_equal(out[0][63 + 65:], want[3][0])
    # BAD_K: k = 1, k = n, k above max_k; BAD_DRAW: a first centre outside the recording
    three = [good[0][0], good[1][0], good[2][0]]
    for ks, max_k, flag in (([3, 1, 3], 3, KR.BAD_K), ([3, 64, 3], 32, KR.BAD_K), ([3, 8, 3], 3, KR.BAD_K)):
        out = _twice(dev, three, ks, draws[:3], max_k=max_k)
        assert out[4].tolist() == [0, flag, 0] and (out[0][63:127] == -1).all(), ks
        assert np.array_equal(out[0][:63], want[0][0]) and np.array_equal(out[0][127:], want[2][0])
    for first in (-1, 64, 2 ** 31 - 1):
        f = draws[1][0].copy()
        f[7] = first
        out = _twice(dev, three, [3, 3, 3], [draws[0], (f, draws[1][1]), draws[2]])
        assert out[4].tolist() == [0, KR.BAD_DRAW, 0] and (out[0][63:127] == -1).all(), first
    # a broken first_row: every recording of the launch is flagged and every label is -1
    for broken in ([0, 70, 63, 192], [0, 63, 127, 193], [1, 63, 127, 192], [0, 63, 127, 191], [0, -5, 127, 192], [0, 63, 2 ** 31 - 1, 192]):
        out = _twice(dev, three, [3, 3, 3], draws[:3], first_row=broken)
        assert out[4].tolist() == [KR.BAD_PROMISE] * 3 and (out[0] == -1).all() and (out[1] == -1).all(), broken


def test_the_drivers_upload_launch_once_and_fall_back(dev):
    from speech_diarization_amd import kmeans_gpu
    cases = KR.gpu_cases(2)[1:5]
    want = _reference("flags", cases)
    deg = KR.degenerate_rows()
    X = np.concatenate([cases[0][0], deg, cases[1][0]])
    states = [np.random.RandomState(cases[0][2]), np.random.RandomState(0), np.random.RandomState(cases[1][2])]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with expect_launches(exactly=KERNELS) as log:
            labels, info = kmeans_gpu.k_means_groups(X, [63, 40, 64], [cases[0][1], 5, cases[1][1]], states, return_info=True)
        host = KR.sklearn_labels(deg, 5, np.random.RandomState(0))[0]
    assert log == {k: 1 for k in KERNELS} and info["fallback"] == [1]
    assert np.array_equal(labels[0], want[0][0]) and np.array_equal(labels[1], host) and np.array_equal(labels[2], want[1][0])
    assert info["iterations"][0] == want[0][2] and info["iterations"][2] == want[1][2]
    # a tensor on the device, a column slice of a wider one, is read in place
    wide = torch.from_numpy(np.pad(cases[2][0], ((0, 0), (0, 3)), constant_values=np.nan)).to(dev)
    with expect_launches(exactly=KERNELS):
        got = kmeans_gpu.k_means_rows(wide[:, :2], cases[2][1], cases[2][2])
    assert np.array_equal(got, want[2][0])
    bad = cases[3][0].copy()
    bad[5, 0] = np.nan
    with expect_launches(exactly=KERNELS):
        with pytest.raises(ValueError, match="contains NaN or infinity"):
            kmeans_gpu.k_means_rows(bad, cases[3][1], 0)


@pytest.mark.parametrize("n,k,noise,seed", [(400, 2, 0.9, 0), (2000, 8, 1.2, 0)])
def test_spectral_with_device_labels_equals_the_sklearn_route(dev, n, k, noise, seed):
    from speech_diarization_amd import cluster_gpu
    X, _ = R.planted_rows(n, k, noise, seed)
    Kd = torch.from_numpy(R.cosine(X).astype(np.float32)).to(dev)
    want = cluster_gpu.spectral(Kd, k)
    with expect_launches(exactly=KERNELS) as log:
        got, info = cluster_gpu.spectral(Kd, k, assign_labels="device", return_info=True)
        again = cluster_gpu.spectral(Kd, k, assign_labels="device")
    assert {kn: log[kn] for kn in KERNELS} == {kn: 2 for kn in KERNELS}
    assert np.array_equal(got, want) and got.dtype == want.dtype and np.array_equal(again, got)
    assert info["kmeans"]["fallback"] is False


def _small_sd(width=128):
    from speech_diarization_amd import synth
    return synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(width))


@pytest.fixture()
def small_encoder(dev):
    from speech_diarization_amd import ecapa_annote, speech_encode
    enc = speech_encode.HipEcapaEncoder(_small_sd(), dev)
    speech_encode.using_ecapa_encoder.cache_clear()
    orig = speech_encode.using_ecapa_encoder
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = lambda device="cuda": enc
    yield enc
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = orig


def test_the_rttm_of_spectral_device_is_that_of_spectral_gpu(small_encoder, tmp_path):
    from speech_diarization_amd import audio_io, diarization_baseline as db, synth
    conv = synth.synthetic_conversation(60.0, 2, seed=0)
    wav = tmp_path / "meeting.wav"
    audio_io.write_wav16(wav, conv.wav, conv.sr)
    seg_g, det_g = db.diarize_audio(wav, 0.35, 0.1, 2, 6, rttm_filepath=tmp_path / "gpu.rttm", clustering="spectral_gpu", return_details=True)
    with expect_launches(exactly=KERNELS) as log:
        seg_d, det_d = db.diarize_audio(wav, 0.35, 0.1, 2, 6, rttm_filepath=tmp_path / "dev.rttm", clustering="spectral_device", return_details=True)
    assert {k: log[k] for k in KERNELS} == {k: 1 for k in KERNELS}
    assert (tmp_path / "dev.rttm").read_bytes() == (tmp_path / "gpu.rttm").read_bytes() and (tmp_path / "dev.rttm").stat().st_size > 0
    assert seg_d == seg_g and np.array_equal(det_d["labels"], det_g["labels"])
    assert {s[2] for s in seg_d} == {"SPEAKER_00", "SPEAKER_01"}
    hp = db.DiarizationParameters(min_speakers=2, max_speakers=6)
    with expect_launches(exactly=KERNELS):
        assert db.Diarizer(hp, clustering="spectral_device").diarize(wav, None) == db.Diarizer(hp, clustering="spectral_gpu").diarize(wav, None)
