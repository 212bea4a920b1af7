"""The device spectral route on the GPU: the two entries of include/sd_hip_spectral.h against f64 numpy over a shape grid, run-to-run
reproducibility, guard bands at exact buffer sizes, and `cluster_gpu` against the host functions end to end and at N = 50 000."""
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import captured as CAP  # noqa: E402
import guarded as G  # noqa: E402
import spectral_ref as R  # noqa: E402
from launch_log import expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message="Graph is not fully connected")

# profiles/spectral_accuracy.json (tools/spectral_accuracy.py on the MI355X): per N of the grid, the largest
# |Y - Y64| / (N 2^-23 (|S| |V|)) over both row strides, both zero_diag values and b in {8, 16, 24, 32}; "apply_max_error_over_bound" is
# the largest of them.  The test bar is 4 x the measurement (accumulation order may change with tile and split choice), and never
# above 1: that is the worst-case f32 bound, and failing it is a bug whatever was measured.
APPLY_MEASURED = {1: 0, 5: 0.200389, 127: 0.0150587, 128: 0.0132924, 129: 0.0135493, 1000: 0.00141835, 3001: 0.00021949}
APPLY_MEASURED_MAX = 0.200389
DEGREE_BAR = 1e-5                # 10 x the log2(N) 2^-24 ~ 1e-6 of a pairwise f32 sum of <= 50 000 non-negative terms


def _dev_affinity(n, ld, dev):
    Kp = R.grid_affinity(n, ld, seed=n)
    return Kp[:, :n], torch.from_numpy(Kp).to(dev)[:, :n]


def test_constants_quote_the_recorded_measurement():
    rec = json.load(open(os.path.join(HERE, "..", "profiles", "spectral_accuracy.json")))
    per_n = {}
    for c in rec["cases"]:
        per_n[c["N"]] = max(per_n.get(c["N"], 0.0), c["error_over_bound"])
    assert set(per_n) == set(R.GRID_N) == set(APPLY_MEASURED)
    for n in R.GRID_N:
        assert APPLY_MEASURED[n] == pytest.approx(per_n[n], rel=1e-3), n
    assert APPLY_MEASURED_MAX == pytest.approx(rec["apply_max_error_over_bound"], rel=1e-3) == pytest.approx(max(per_n.values()), rel=1e-3)
    assert rec["apply_max_error_over_bound"] <= 1.0 and rec["degree_max_rel_err"] <= DEGREE_BAR


@pytest.mark.parametrize("n", R.GRID_N)
def test_degree_against_f64(dev, n):
    from speech_diarization_amd import ops
    for ld in R.grid_lds(n):
        K, Kd = _dev_affinity(n, ld, dev)
        for zd in (False, True):
            ref = R.degree_ref(K, zd)
            with expect_launches(exactly=["affinity_degree_kernel"]):
                deg = ops.affinity_degree(Kd, zd).cpu().numpy().astype(np.float64)
            rel = np.abs(deg - ref) / np.where(ref > 0, ref, 1.0)
            print(f"degree N={n} ld={ld} zero_diag={zd}: max rel err {rel.max():.3e}")
            assert np.all(np.isfinite(deg)) and rel.max() <= DEGREE_BAR
            assert np.all(deg[ref == 0] == 0)
            if n >= 5:
                assert (ref == 0).sum() >= 1                   # the grid has rows without a positive entry


@pytest.mark.parametrize("n", R.GRID_N)
def test_apply_against_f64(dev, n):
    from speech_diarization_amd import ops
    worst = 0.0
    for ld in R.grid_lds(n):
        K, Kd = _dev_affinity(n, ld, dev)
        for zd in (False, True):
            scale = R.grid_scale(K, zd)
            for b in R.GRID_B:
                V = R.grid_block(n, b, seed=n + b)
                # one or two blocks of 16 columns per thread; 16-byte loads of K when its rows are 16-byte aligned, scalar ones otherwise
                with expect_launches(exactly=[f"affinity_apply_kernel<{1 if b <= 16 else 2},{'vec' if ld % 4 == 0 else 'scalar'}>", "apply_finish_kernel"]):
                    Y = ops.affinity_apply(Kd, torch.from_numpy(scale).to(dev), torch.from_numpy(V).to(dev), zd).cpu().numpy()
                r = R.apply_error_over_bound(Y, K, scale, V, zd)
                print(f"apply N={n} ld={ld} zero_diag={zd} b={b}: error / bound {r:.4f}")
                assert np.all(np.isfinite(Y))
                assert r <= 1.0, "outside the worst-case f32 bound N 2^-23 (|S| |V|): a bug"
                worst = max(worst, r)
    assert worst <= min(1.0, 4.0 * APPLY_MEASURED[n]) and worst <= min(1.0, 4.0 * APPLY_MEASURED_MAX)


def test_entries_are_bitwise_reproducible(dev):
    from speech_diarization_amd import ops
    for n in (129, 3001):
        ld = R.grid_lds(n)[1]
        K, Kd = _dev_affinity(n, ld, dev)
        scale = torch.from_numpy(R.grid_scale(K, True)).to(dev)
        for zd in (False, True):
            d = [ops.affinity_degree(Kd, zd) for _ in range(2)]
            assert torch.equal(d[0], d[1])
            for b in (16, 32):
                V = torch.from_numpy(R.grid_block(n, b, 1)).to(dev)
                y = [ops.affinity_apply(Kd, scale, V, zd) for _ in range(2)]
                assert torch.equal(y[0], y[1])


def test_lib_refuses_on_the_device_too(dev):
    """The refusals of tests/test_spectral_rules.py with real device buffers: nothing is written."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    K = torch.ones((64, 64), device=dev)
    s = torch.ones(64, device=dev)
    V = torch.ones((64, 16), device=dev)
    Y = torch.full((64, 16), 7.0, device=dev)
    ws = torch.empty(int(lib.sd_affinity_apply_workspace_bytes(64, 16)), dtype=torch.uint8, device=dev)
    args = lambda b=16, nbytes=ws.numel(): (K.data_ptr(), 64, 64, 0, s.data_ptr(), V.data_ptr(), 16, b, Y.data_ptr(), 16, ws.data_ptr(), nbytes, None)  # noqa: E731
    assert lib.sd_affinity_apply_f32(*args(b=12)) == -2
    assert lib.sd_affinity_apply_f32(*args(nbytes=ws.numel() - 256)) == -3
    torch.cuda.synchronize()
    assert bool((Y == 7.0).all())
    assert lib.sd_affinity_apply_f32(*args()) == 0
    torch.cuda.synchronize()
    assert float(Y[0, 0]) == 64.0


# ------------------------------------------------------------------ exact buffer sizes, guard bands (style of test_gpu_buffer_edges.py)

def _edge_degree(dev, n, ld, zd, poison):
    from speech_diarization_amd import _native as N
    K = R.grid_affinity(n, ld, seed=n)
    flat = torch.from_numpy(K.reshape(-1)[: (n - 1) * ld + n].copy())
    gK = G.guarded_from(flat, dev, "K")                           # the last row ends at its last column: no padding behind it
    gd = G.guarded(n * 4, poison, dev, "deg")
    N.check(CAP.call("sd_affinity_degree_f32", gK.ptr, n, ld, int(zd), gd.ptr), "sd_affinity_degree_f32")
    torch.cuda.synchronize()
    G.assert_guards_intact(gK, gd)
    return gd.view(torch.float32).clone()


def _edge_apply(dev, n, ld, zd, b, ldv, ldy, poison):
    from speech_diarization_amd import _native as N
    lib = N.load()
    K = R.grid_affinity(n, ld, seed=n)
    gK = G.guarded_from(torch.from_numpy(K.reshape(-1)[: (n - 1) * ld + n].copy()), dev, "K")
    gs = G.guarded_from(torch.from_numpy(R.grid_scale(K[:, :n], zd)), dev, "scale")
    V = np.full((n, ldv), np.nan, np.float32)
    V[:, :b] = R.grid_block(n, b, 3)
    gV = G.guarded_from(torch.from_numpy(V.reshape(-1)[: (n - 1) * ldv + b].copy()), dev, "V")
    gY = G.guarded(((n - 1) * ldy + b) * 4, poison, dev, "Y")
    need = int(lib.sd_affinity_apply_workspace_bytes(n, b))
    gw = G.guarded(need, poison, dev, "ws")
    N.check(CAP.call("sd_affinity_apply_f32", gK.ptr, n, ld, int(zd), gs.ptr, gV.ptr, ldv, b, gY.ptr, ldy, gw.ptr, need), "sd_affinity_apply_f32")
    torch.cuda.synchronize()
    G.assert_guards_intact(gK, gs, gV, gY, gw)
    y = gY.view(torch.float32)
    full = torch.cat([y, torch.zeros(ldy - b, dtype=torch.float32, device=y.device)]).view(n, ldy) if ldy > b else y.view(n, ldy)
    if ldy > b and n > 1:                                          # the columns between the rows keep the poison
        pad = gY.payload[: (n - 1) * ldy * 4].view(n - 1, ldy * 4)[:, b * 4:]
        assert bool((pad == poison).all()), "Y: columns [b, ldy) written"
    return full[:, :b].clone()


EDGE_SHAPES = [(1, 1), (1, 4), (5, 8), (129, 131), (129, 132), (1000, 1000), (1000, 1003)]      # (N, ld): ld == N, odd, multiple of 4


@pytest.mark.parametrize("n,ld", EDGE_SHAPES)
def test_degree_at_exact_buffer_sizes(dev, n, ld):
    from speech_diarization_amd import ops
    Kd = torch.from_numpy(R.grid_affinity(n, ld, seed=n)).to(dev)[:, :n]
    for zd in (False, True):
        want = ops.affinity_degree(Kd, zd)
        for poison in G.POISONS:
            assert torch.equal(_edge_degree(dev, n, ld, zd, poison), want), (zd, poison)


@pytest.mark.parametrize("n,ld", EDGE_SHAPES)
def test_apply_at_exact_buffer_sizes(dev, n, ld):
    from speech_diarization_amd import ops
    Kp = R.grid_affinity(n, ld, seed=n)
    Kd = torch.from_numpy(Kp).to(dev)[:, :n]
    for zd in (False, True):
        scale = torch.from_numpy(R.grid_scale(Kp[:, :n], zd)).to(dev)
        for b in R.GRID_B:
            want = ops.affinity_apply(Kd, scale, torch.from_numpy(R.grid_block(n, b, 3)).to(dev), zd)
            assert bool(torch.isfinite(want).all())
            for (ldv, ldy), poison in zip(((b, b), (b + 3, b + 5), (b + 1, b)), G.POISONS):
                assert torch.equal(_edge_apply(dev, n, ld, zd, b, ldv, ldy, poison), want), (zd, b, ldv, ldy, poison)


# ------------------------------------------------------------------ end to end

def _small_sd(width=128):
    from speech_diarization_amd import synth
    return synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(width))


def test_meeting_count_and_partition_equal_the_host_functions(dev):
    """10 min, 8 voices, small weights, every window (n > 1000): the affinity never leaves the device on the new route; the host
    functions get its copy."""
    from speech_diarization_amd import cluster, cluster_gpu, ops, synth, vad
    from speech_diarization_amd.diarization_baseline import gather_windows, speech_windows
    from speech_diarization_amd.engine import EmbeddingEngine
    conv = synth.synthetic_conversation(600.0, 8, seed=0)
    scorer = vad.SileroVAD(model=vad.EnergyScorer())
    mask = vad.morph_open_close(vad.hysteresis_binarize(scorer.probs(conv.wav), 0.6, 0.4), 10.0)
    speech = vad.mask_to_segments(mask, 10.0, 350.0, 100.0, 40.0)
    starts, _, _ = speech_windows(speech, len(conv.wav), 16000, 2.0, 0.25)
    wav = torch.from_numpy(gather_windows(conv.wav, starts, 32000)).to(dev)
    n = wav.shape[0]
    assert n > 1000
    emb = EmbeddingEngine(_small_sd(), dev, max_batch=256).embed(wav).cpu().numpy()
    Kd = ops.cosine_affinity(torch.from_numpy(cluster.center(emb).astype(np.float32)).to(dev))
    assert torch.equal(Kd, Kd.T)                                   # what assume_symmetric relies on
    K = Kd.cpu().numpy()
    for lo, hi in ((2, 8), (2, 12), (1, 10)):
        got, info = cluster_gpu.estimate_num_speakers(Kd, lo, hi, return_info=True)
        print(f"n={n} [{lo}, {hi}]: {got} speakers, {info['passes']} passes, residual {info['residual']:.2e}")
        assert got == cluster.estimate_num_speakers(K, lo, hi)
    runs = [cluster_gpu.spectral(Kd, 8, assume_symmetric=sym) for sym in (True, False, True)]
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])        # equal labels run to run
    got = cluster.relabel_by_first_appearance(runs[0])
    want = cluster.relabel_by_first_appearance(cluster.spectral(K, 8))
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {n} labels differ"
    assert len(set(got.tolist())) == 8
    # an affinity that is not symmetric is symmetrised as the host functions do it
    Ka = Kd.clone()
    Ka[0, 1] += 0.25
    got = cluster.relabel_by_first_appearance(cluster_gpu.spectral(Ka, 8))
    assert np.array_equal(got, cluster.relabel_by_first_appearance(cluster.spectral(Ka.cpu().numpy(), 8)))


@pytest.fixture()
def small_encoder(dev):
    from speech_diarization_amd import ecapa_annote, speech_encode
    enc = speech_encode.HipEcapaEncoder(_small_sd(), dev)
    speech_encode.using_ecapa_encoder.cache_clear()
    orig = speech_encode.using_ecapa_encoder
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = lambda device="cuda": enc
    yield enc
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = orig


def test_config0_rttm_is_byte_identical_on_the_device_route(small_encoder, tmp_path):
    from speech_diarization_amd import audio_io, diarization_baseline as db, synth
    conv = synth.synthetic_conversation(60.0, 2, seed=0)
    wav = tmp_path / "meeting.wav"
    audio_io.write_wav16(wav, conv.wav, conv.sr)
    seg_h, det_h = db.diarize_audio(wav, 0.35, 0.1, 2, 6, rttm_filepath=tmp_path / "host.rttm", clustering="spectral", return_details=True)
    seg_d, det_d = db.diarize_audio(wav, 0.35, 0.1, 2, 6, rttm_filepath=tmp_path / "dev.rttm", clustering="spectral_gpu", return_details=True)
    assert (tmp_path / "dev.rttm").read_bytes() == (tmp_path / "host.rttm").read_bytes()
    assert seg_d == seg_h and np.array_equal(det_d["labels"], det_h["labels"])
    assert isinstance(det_d["affinity"], np.ndarray) and np.array_equal(det_d["affinity"], det_h["affinity"])
    assert {s[2] for s in seg_d} == {"SPEAKER_00", "SPEAKER_01"}
    # the same string through the Diarizer
    hp = db.DiarizationParameters(min_speakers=2, max_speakers=6)
    assert db.Diarizer(hp, clustering="spectral_gpu").diarize(wav, None) == db.Diarizer(hp, clustering="spectral").diarize(wav, None)


def test_scale_50k_rows_12_planted_speakers(dev):
    """No host reference exists at this size (a 20 GB f64 copy and a dense N^3 solve): the check is against the planted labels."""
    from speech_diarization_amd import cluster, cluster_gpu, ops
    n, k = 50000, 12
    X, planted = R.planted_rows(n, k, 0.9, seed=0, dtype=np.float32)
    Kd = ops.cosine_affinity(torch.from_numpy(X).to(dev))
    got_k, info = cluster_gpu.estimate_num_speakers(Kd, 1, 16, assume_symmetric=True, return_info=True)
    print(f"N={n}: {got_k} speakers, {info['passes']} passes, residual {info['residual']:.2e}, gaps {np.diff(info['eigenvalues'])[:14]}")
    assert got_k == k
    labels, info = cluster_gpu.spectral(Kd, k, assume_symmetric=True, return_info=True)
    print(f"N={n}: spectral {info['passes']} passes, residual {info['residual']:.2e}")
    assert np.array_equal(cluster.relabel_by_first_appearance(labels), cluster.relabel_by_first_appearance(planted))
