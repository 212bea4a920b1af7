"""No-GPU checks of the "VBx-like" diarizer (speech-diarization_amd/diar_diag.py) against the reference's own `main`, recorded by
tests/golden/make_diag_golden.py with scripted doubles (tests/helpers/diag_cases.py): the context spans, the three output files byte
for byte on the host route, the tool's private VAD helpers, and the driver of diag_gpu over a numpy operator against
`cluster.whiten_l2`."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import diag_cases as DC  # noqa: E402

from speech_diarization_amd import cluster, diag_gpu  # noqa: E402
from speech_diarization_amd import diar_diag as dd  # noqa: E402


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "diar_diag_pipeline.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def conv(golden):
    c = DC.conversation()
    p = golden["pipeline"]
    assert len(c.wav) == p["n_samples"] and float(np.abs(c.wav.astype(np.float64)).sum()) == p["wav_abs_sum"]    # the recorded recording
    return c


def _bools(s):
    return np.frombuffer(s.encode(), np.uint8) == ord("1")


def _vad_segments(case, conv, golden):
    segs = DC.scripted_segments(case["segs"], conv.turns, DC.CONVERSATION["duration_s"])
    probs = DC.probs_from_segments(segs, golden["pipeline"]["n_frames"])
    mask = dd.morph_open_close(dd.hysteresis_binarize(probs), 10.0)
    return segs, probs, dd.mask_to_segments(mask, 10.0)


# ------------------------------------------------------------------ spans

def test_the_cases_are_the_recorded_ones(golden):
    cases = DC.pipeline_cases()
    assert set(cases) == set(golden["pipeline"]["cases"]) and len(cases) == 19
    for name, c in cases.items():
        g = golden["pipeline"]["cases"][name]
        assert g["kwargs"] == {k: v for k, v in c.items() if k not in ("segs", "rows")} and g["segs"] == c["segs"] and g["rows"] == c["rows"]


@pytest.mark.parametrize("name", ["agglo_w0_a0_v0", "tiled_no_context", "clamped_at_both_ends"])
def test_context_spans_are_the_pieces_the_reference_embedded(golden, conv, name):
    g = golden["pipeline"]["cases"][name]
    _, _, segs = _vad_segments(g, conv, golden)
    spans = golden["pipeline"]["spans"][g["spans"]]
    assert len(segs) == len(spans)
    starts, lengths, tile_to = dd.context_spans(segs, len(conv.wav), DC.SR, g["kwargs"].get("pad_ctx", 0.2))
    floor = int(0.4 * DC.SR)
    for i, (off, length) in enumerate(spans):
        if off < 0:                                                  # a tiled copy: exactly int(0.4 sr) samples of a shorter piece
            assert tile_to[i] == floor == length and lengths[i] < floor, i
        else:
            assert (starts[i], lengths[i], tile_to[i]) == (off, length, 0), i
    tiled = [i for i, (off, _) in enumerate(spans) if off < 0]
    assert (len(tiled) == 1) == (name == "tiled_no_context")
    if name == "clamped_at_both_ends":
        assert starts[0] == 0 and starts[-1] + lengths[-1] == len(conv.wav)
        assert segs[0][0] - 0.2 < 0 and segs[-1][1] + 0.2 > len(conv.wav) / DC.SR


def test_tiled_piece_is_the_reference_tiling():
    y = np.arange(1, 20001, dtype=np.float32)
    enc = DC.ScriptedEncoder(np.ones((2, 4), np.float32))
    seen = []
    enc._one = lambda a: seen.append(np.array(a)) or np.zeros(4, np.float32)
    dd.embed_segments_with_context(y, DC.SR, [[0.5, 0.65], [0.1, 1.0]], pad_ctx=0.0, encoder=enc)
    a = y[8000:10400]
    assert np.array_equal(seen[0], np.tile(a, 3)[:6400]) and np.array_equal(seen[1], y[1600:16000])
    with pytest.raises(ValueError, match="no sample"):
        dd.context_spans([[5.0, 5.5]], 20000, DC.SR, 0.2)


# ------------------------------------------------------------------ the three files, byte for byte

def _run(name, golden, conv, tmp_path, **extra):
    g = golden["pipeline"]["cases"][name]
    segs, probs, _ = _vad_segments(g, conv, golden)
    enc = DC.ScriptedEncoder(DC.scripted_rows(g["rows"], len(segs)))
    res = dd.diagnose(conv.wav, DC.SR, probs, encoder=enc, device=None, out_dir=str(tmp_path), **g["kwargs"], **extra)
    return g, enc, res


@pytest.mark.parametrize("name", sorted(DC.pipeline_cases()))
def test_host_route_reproduces_the_reference_files(golden, conv, tmp_path, name):
    g, enc, res = _run(name, golden, conv, tmp_path)
    assert [n for n, _ in enc.log] == [length for _, length in golden["pipeline"]["spans"][g["spans"]]]
    raw = {kind: open(res["paths"][kind], "rb").read() for kind in ("json", "srt", "csv")}
    assert raw["csv"].decode("utf-8") == g["csv"], name               # the csv as text; the other two files by the hash of their bytes
    assert hashlib.sha256(raw["json"]).hexdigest() == g["json_sha256"] and hashlib.sha256(raw["srt"]).hexdigest() == g["srt_sha256"], name
    n = len(res["vad_segments"])
    assert res["adjacent"].shape == (n - 1,) and np.all(np.abs(res["adjacent"]) <= 1 + 1e-6) and res["nonadjacent"].size > 0
    assert res["final_labels"].shape == (n,) and res["scores"].shape == (n, len(res["centers"]))


def test_all_noise_falls_back_to_one_centre(golden, conv, tmp_path):
    seen = []

    def factory(**kw):
        inner = cluster.default_hdbscan_factory(**kw)

        class Spy:
            def fit_predict(self, D):
                seen.append(np.asarray(inner.fit_predict(D)))
                return seen[-1]
        return Spy()
    _, _, res = _run("all_noise", golden, conv, tmp_path, clusterer_factory=factory)
    assert len(seen) == 1 and np.all(seen[0] == -1)
    assert np.all(res["labels"] == 0) and res["centers"].shape == (1, DC.D) and res["speakers"] == ["SPK_0"]


def test_resegment_argument_checks():
    X, _ = DC.planted_lowrank(12, 2, 3, 0.2, 0)
    segs = [[i * 1.0, i * 1.0 + 0.5] for i in range(12)]
    with pytest.raises(ValueError, match="hdbscan"):
        dd.resegment(X, segs, cluster="kmeans")
    with pytest.raises(ValueError, match="segments"):
        dd.resegment(X, segs[:-1])
    with pytest.raises(ValueError, match="host route"):
        dd.resegment(X, segs, device="cuda", clusterer_factory=lambda **kw: None)
    with pytest.raises(ValueError, match="device route"):
        dd.resegment(X, segs, operator=DC.NumpyDiag())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dd.resegment(X, segs, device="cpu")
    with pytest.raises(NotImplementedError, match="speechbrain-ecapa"):
        dd.main("x.wav", backend="ali-campp")
    with pytest.raises(ValueError, match="no speech segment"):
        dd.diagnose(np.zeros(16000, np.float32), DC.SR, np.zeros(98, np.float32), encoder=DC.ScriptedEncoder(X))


def test_dropin_shim_binds_the_pipeline():
    import importlib
    path = os.path.join(os.path.dirname(HERE), "dropin")
    sys.path.insert(0, path)
    try:
        sys.modules.pop("diar_diag", None)
        mod = importlib.import_module("diar_diag")
        assert mod.main is dd.main and mod.resegment is dd.resegment and mod.whiten_l2 is cluster.whiten_l2
    finally:
        sys.path.remove(path)
        sys.modules.pop("diar_diag", None)


# ------------------------------------------------------------------ the tool's private VAD helpers

def test_mask_to_segments_equals_the_reference_on_200_masks(golden):
    masks = golden["vad"]["masks"]
    assert len(masks) == 200
    kept = 0
    for c in masks:
        got = dd.mask_to_segments(DC.mask_from_runs(c["runs"]), c["hop_ms"], c["min_speech_ms"], c["min_gap_ms"])
        assert got == c["segments"], c                                # float for float: nothing is rounded
        kept += len(got)
    assert kept > 150
    assert dd.mask_to_segments(np.zeros(0, bool), 10.0) == [] and dd.mask_to_segments(np.zeros(50, bool), 10.0) == []


def test_hysteresis_and_morphology_equal_the_reference(golden):
    for track in golden["vad"]["tracks"]:
        probs = np.asarray(track["probs"], np.float32)
        for v in track["variants"]:
            h = dd.hysteresis_binarize(probs, v["on"], v["off"])
            assert np.array_equal(h, _bools(v["hyst"]))
            assert np.array_equal(dd.morph_open_close(h, 10.0, v["open_ms"], v["close_ms"]), _bools(v["mask"]))


def test_framing_and_context_equal_the_reference(golden):
    for c in golden["vad"]["frames"]:
        f, hop = dd.frame_audio(np.arange(c["n"], dtype=np.float32), c["sr"], c["win_ms"], c["hop_ms"])
        assert list(f.shape) == c["shape"] and hop == c["hop"]
        assert f[0][:3].tolist() == c["first"] and f[-1][-3:].tolist() == c["last"]
    y = np.arange(48000, dtype=np.float32)
    for c in golden["vad"]["context"]:
        a = dd.pad_with_context(y, 16000, c["start"], c["end"], ctx=c["ctx"])
        assert (int(a[0]), len(a)) == (c["first"], c["length"])
        s, n, _ = dd.context_spans([[c["start"], c["end"]]], len(y), 16000, c["ctx"])
        assert (int(s[0]), int(n[0])) == (c["first"], c["length"])


def test_conditioning(tmp_path):
    from speech_diarization_amd import audio_io
    y = (0.1 * np.sin(np.arange(32000) / 7.0) + 0.02).astype(np.float32)
    audio_io.write_wav16(tmp_path / "a.wav", y, 16000)
    x, sr = audio_io.read_audio(tmp_path / "a.wav")
    got, sr2 = dd.load_audio(str(tmp_path / "a.wav"))
    xc = x.astype(np.float64) - x.astype(np.float64).mean()
    assert sr2 == sr == 16000 and got.dtype == np.float32
    assert np.array_equal(got[1:], (xc[1:] - 0.97 * xc[:-1]).astype(np.float32))
    z = dd.loudness_normalize(got * 50.0, sr)
    assert np.abs(z).max() <= 0.99 and np.array_equal(dd.loudness_normalize(np.full(10, 2.0), sr), np.full(10, 0.99))


# ------------------------------------------------------------------ the driver of diag_gpu on the CPU

@pytest.mark.parametrize("n", [40, 300, 2000])
@pytest.mark.parametrize("kind", ["planted", "isotropic"])
def test_driver_over_the_numpy_operator_equals_whiten_l2(n, kind):
    """Rows within 1e-8: the operator's f64 sums are numpy's in another order (measured <= 1.3e-9) and its result is rounded to f32
    once, so the comparison is made before that rounding, on the operator's f64 value."""
    if kind == "planted":
        X, _ = DC.planted_lowrank(n, 4, 8, 0.3, n)
    else:
        X = (np.random.default_rng(n).standard_normal((n, DC.D)) * 30.0).astype(np.float32)

    class F64(DC.NumpyDiag):
        def apply(self, X, mean, W):
            v = (X.numpy().astype(np.float64) - mean.numpy()) @ W.numpy()
            self.v = v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-9)
            return super().apply(X, mean, W)
    op = F64()
    got = diag_gpu.whiten_l2_rows(torch.from_numpy(X), operator=op)
    want = cluster.whiten_l2(X)
    assert op.calls == ["stats", "apply"] and got.dtype == torch.float32 and tuple(got.shape) == X.shape
    err = np.abs(op.v - want).max()
    print(f"n={n} {kind}: max |row - whiten_l2| = {err:.2e}")
    assert err <= 1e-8
    assert np.abs(got.numpy() - want).max() <= 1e-8 + 2.0 ** -25
    assert np.abs(got.numpy().astype(np.float64) @ got.numpy().astype(np.float64).T - want @ want.T).max() <= 1e-6


def test_driver_refusals():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diag_gpu.whiten_l2_rows(torch.ones(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diag_gpu.whiten_l2_rows(np.ones((4, 8), np.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diag_gpu.DeviceDiag("cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diag_gpu.label_centroids_rows(torch.ones(4, 8), torch.zeros(4, dtype=torch.int32), 1)
    op = DC.NumpyDiag()
    with pytest.raises(ValueError, match="two rows"):
        diag_gpu.whiten_l2_rows(torch.ones(1, 8), operator=op)
    bad = torch.ones(4, 8)
    bad[2, 3] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        diag_gpu.whiten_l2_rows(bad, operator=op)
    with pytest.raises(ValueError, match="k must be"):
        diag_gpu.label_centroids_rows(torch.ones(4, 8), torch.zeros(4, dtype=torch.int32), 1025, operator=op)
    assert op.calls == []
    from speech_diarization_amd import ops
    for call in (lambda: ops.whiten_stats(torch.ones(4, 8)), lambda: ops.whiten_apply(torch.ones(4, 8), torch.zeros(8, dtype=torch.float64), torch.eye(8, dtype=torch.float64)),
                 lambda: ops.label_centroids(torch.ones(4, 8), torch.zeros(4, dtype=torch.int32), 1), lambda: ops.rows_product(torch.ones(4, 8), torch.ones(2, 8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_centroids_over_the_numpy_operator_equal_the_reference_loop():
    X, lab = DC.planted_lowrank(60, 3, 6, 0.3, 7)
    lab = lab.copy()
    lab[::7] = -1
    cen, count = diag_gpu.label_centroids_rows(torch.from_numpy(X), torch.from_numpy(lab), 4, operator=DC.NumpyDiag())
    for k in range(3):
        m = X[lab == k].astype(np.float64).mean(0)
        assert np.abs(cen[k].numpy() - m / (np.linalg.norm(m) + 1e-9)).max() <= 2.0 ** -24
    assert count.tolist() == [int((lab == k).sum()) for k in range(3)] + [0] and not cen[3].any()
