"""BASELINE.json configs[0]: the diarization_baseline entry point on a 60 s 2-speaker synthetic WAV
with a PyTorch-CPU ECAPA (the oracle, injected as `encoder=`) and spectral clustering — plumbing,
no GPU.  Checks the output schema (segment tuples, RTTM lines), speaker count and turn boundaries.
The GPU twin of this test (tests/test_gpu_pipeline.py) must produce the identical RTTM."""
import numpy as np
import pytest
import torch

from speech_diarization_amd import audio_io, diarization_baseline as db, rttm, synth


@pytest.fixture(scope="module")
def conversation(tmp_path_factory):
    conv = synth.synthetic_conversation(60.0, n_speakers=2, seed=0)
    path = tmp_path_factory.mktemp("cfg0") / "meeting.wav"
    audio_io.write_wav16(path, conv.wav, conv.sr)
    return conv, path


def cpu_oracle_encoder(width=128, seed=1234, sd=None):
    from oracle.ecapa_ref import EcapaRef
    from oracle.pipeline_ref import encode_batch_ref
    sd = synth.make_ecapa_state_dict(seed, synth.EcapaConfig.small(width)) if sd is None else sd
    net = EcapaRef(sd, torch.float32)
    return lambda wavs: encode_batch_ref(sd, np.asarray(wavs, np.float32), torch.float32, net).astype(np.float32)


def test_config0_plumbing(conversation, tmp_path):
    conv, path = conversation
    out_rttm = tmp_path / "meeting.rttm"
    segments, det = db.diarize_audio(path, 0.35, 0.1, 2, 6, rttm_filepath=out_rttm, encoder=cpu_oracle_encoder(),
                                     clustering="spectral", return_details=True)
    # schema: (start_s, end_s, "SPEAKER_xx") tuples, sorted, non-empty
    assert segments and all(len(s) == 3 and isinstance(s[2], str) and s[2].startswith("SPEAKER_") and s[1] > s[0] for s in segments)
    assert {s[2] for s in segments} == {"SPEAKER_00", "SPEAKER_01"}
    lines = out_rttm.read_text().splitlines()
    assert len(lines) == len(segments)
    for ln, (s, e, k) in zip(lines, segments):
        f = ln.split()
        assert f[0] == "SPEAKER" and f[1] == "meeting" and f[2] == "1" and f[5:7] == ["<NA>", "<NA>"] and f[7] == k and f[8:] == ["<NA>", "<NA>"]
        assert abs(float(f[3]) - s) < 1e-3 and abs(float(f[4]) - (e - s)) < 2e-3
    assert rttm.read_rttm(out_rttm) == [(pytest.approx(s, abs=1e-3), pytest.approx(e, abs=2e-3), k) for s, e, k in segments]
    # the two synthetic voices are recovered: DER against the ground-truth turns is small
    truth = [(s, e, f"T{k}") for s, e, k in conv.turns]
    assert rttm.der(truth, segments) < 0.10
    # every true turn boundary has a hypothesis boundary within 0.25 s
    hyp_edges = np.array([s for s, _, _ in segments] + [e for _, e, _ in segments])
    for s, e, _ in conv.turns:
        assert np.abs(hyp_edges - s).min() < 0.25 and np.abs(hyp_edges - e).min() < 0.25
    assert det["embeddings"].shape[1] == 192 and len(det["labels"]) == det["embeddings"].shape[0]


def test_diarizer_end_to_end_writes_stems(conversation, tmp_path):
    conv, path = conversation
    hp = db.DiarizationParameters(min_speakers=2, max_speakers=4, fade_ms=30.0, same_speaker_gap_s=1.0)
    d = db.Diarizer(hp, encoder=cpu_oracle_encoder(64))
    segments, info = d(path, tmp_path / "meeting-speakers", with_rttm=False)
    assert len({k for _, _, k in segments}) == 2
    assert set(info) == {k for _, _, k in segments}
    for spk, files in info.items():
        assert files and all(f.endswith(".flac") and f"/{spk}/meeting-" in f for f in files)
        for f in files:
            y, sr = audio_io.read_audio(f, 16000, mono=True)
            assert 3.0 <= len(y) / sr <= hp.max_segment_s + 1e-6


def test_segment_glue_units():
    segs = [(0.0, 1.0, "A"), (1.5, 2.0, "A"), (4.0, 5.0, "A"), (5.1, 6.0, "B")]
    assert db.merge_same_speaker(segs, 1.2, 20) == [(0.0, 2.0, "A"), (4.0, 5.0, "A"), (5.1, 6.0, "B")]
    assert db.adjust_segment_boundaries([(0, 1, "A"), (1.5, 2, "A"), (2.01, 3, "B")], 0.04) == [(0, 1.04, "A"), (1.46, 2, "A"), (2.01, 3, "B")]
    plans = db.plan_speaker_tracks([(0.0, 8.0, "A"), (9.0, 15.0, "A"), (30.0, 41.0, "A")], max_segment_s=20.0, max_gap_s=1.5)
    assert plans["A"] == [[("speech", 0.0, 8.0), ("silence", 1.0), ("speech", 9.0, 15.0)], [("speech", 30.0, 41.0)]]
    assert db.expand_audios.__name__ == "expand_audios"


def test_der_scorer():
    ref = [(0.0, 5.0, "a"), (5.0, 10.0, "b")]
    assert rttm.der(ref, [(0.0, 5.0, "x"), (5.0, 10.0, "y")]) == 0.0          # label names do not matter
    assert rttm.der(ref, [(0.0, 10.0, "x")]) == pytest.approx(0.5, abs=0.01)   # one speaker confused
    assert rttm.der(ref, [(0.0, 5.0, "x")]) == pytest.approx(0.5, abs=0.01)    # half missed
    assert rttm.der(ref, ref) == 0.0 and rttm.der([], []) == 0.0


def test_streaming_ring_is_written_in_place_and_reads_the_last_window():
    """configs[3] host logic without a GPU: the doubled ring of `StreamingEmbedder` (two hop-sized in-place copies per
    hop, window start offset = write position) hands `embed_windows` exactly the last `window_s` of every channel."""
    import torch
    from speech_diarization_amd.streaming import StreamingEmbedder

    class StubEngine:
        device = torch.device("cpu")

        def __init__(self):
            self.seen = []

        def embed_windows(self, signal, starts, n):
            rows = torch.stack([signal[int(s): int(s) + n] for s in starts])
            self.seen.append(rows.clone())
            return rows[:, :192].clone()

    eng = StubEngine()
    st = StreamingEmbedder(eng, channels=3, window_s=0.5, hop_s=0.125, sr=1600, use_graph=False)   # win 800, hop 200
    buf_ptr = st._buf.data_ptr()
    rng = np.random.default_rng(0)
    feed = rng.standard_normal((3, 200 * 11)).astype(np.float32)
    for h in range(11):
        out = st.push(torch.from_numpy(feed[:, h * 200:(h + 1) * 200]))
        want = np.zeros((3, 800), np.float32)
        have = feed[:, max(0, (h + 1) * 200 - 800):(h + 1) * 200]
        want[:, 800 - have.shape[1]:] = have
        assert np.array_equal(eng.seen[-1].numpy(), want) and np.array_equal(st.ring.numpy(), want)
        assert out.shape == (3, 192)
    assert st._buf.data_ptr() == buf_ptr                       # never re-allocated
    with pytest.raises(ValueError):
        st.push(torch.zeros(3, 7))
    # a window that is NOT a whole number of hops: the hop wraps around the end of the ring
    st = StreamingEmbedder(eng, channels=2, window_s=0.5, hop_s=0.3, sr=1000, use_graph=False)     # win 500, hop 300
    feed = rng.standard_normal((2, 300 * 9)).astype(np.float32)
    for h in range(9):
        st.push(torch.from_numpy(feed[:, h * 300:(h + 1) * 300]))
        want = np.zeros((2, 500), np.float32)
        have = feed[:, max(0, (h + 1) * 300 - 500):(h + 1) * 300]
        want[:, 500 - have.shape[1]:] = have
        assert np.array_equal(eng.seen[-1].numpy(), want) and np.array_equal(st.ring.numpy(), want), h
    for bad in (0.0, 0.6):
        with pytest.raises(ValueError):
            StreamingEmbedder(eng, channels=1, window_s=0.5, hop_s=bad, sr=1600, use_graph=False)


def test_windows_read_in_place_are_the_rows_the_host_path_gathers(monkeypatch, tmp_path):
    """The GPU path of SCD and of `diarize_audio` hands `encode_windows` a signal and START OFFSETS instead of gathered rows
    (`sd_fbank_windows_f32` reads the windows in place).  Without a GPU: a stand-in encoder behind `using_ecapa_encoder` that gathers
    `signal[s : s + n]` itself (zero padded) must give exactly what the literal host path gives — i.e. the offsets are the rows of
    `frame_audio` / `gather_windows`."""
    from speech_diarization_amd import anti_stick_diarize as asd, speech_encode

    def cpu_encode(w):
        w = np.asarray(w, dtype=np.float32)
        return np.stack([np.abs(np.fft.rfft(r, 382))[:192] for r in w]).astype(np.float32)

    class FakeEncoder:
        def __init__(self):
            self.calls = []

        def encode_windows(self, signal, starts, n, rows_per_call=8192, to_host=True):
            signal = np.asarray(signal, dtype=np.float32)
            rows = np.zeros((len(starts), n), np.float32)
            for i, s in enumerate(np.asarray(starts)):
                piece = signal[int(s): int(s) + n]
                rows[i, : len(piece)] = piece
            self.calls.append((len(signal), len(starts), n))
            return cpu_encode(rows)

    fake = FakeEncoder()
    monkeypatch.setattr(speech_encode, "using_ecapa_encoder", lambda device="cuda": fake)
    host_cos = asd.adjacent_cosine
    monkeypatch.setattr(asd, "adjacent_cosine", lambda e, use_gpu: host_cos(e, False))
    conv = synth.synthetic_conversation(40.0, 3, seed=4)
    segs = [asd.Segment(0.37, 9.81), asd.Segment(10.2, 10.9), asd.Segment(12.0, 31.456), asd.Segment(33.3, 39.99)]
    a = asd.scd_split_segments(conv.wav, 16000, segs, thr=1.0)                       # "GPU" path: offsets
    b = asd.scd_split_segments(conv.wav, 16000, segs, thr=1.0, encode=cpu_encode)    # host path: frame_audio rows
    assert [(s.start, s.end) for s in a] == [(s.start, s.end) for s in b] and len(a) > len(segs)
    assert len(fake.calls) == 1 and fake.calls[0][0] == len(conv.wav) and fake.calls[0][2] == 16000   # ONE call, the whole signal
    # diarize_audio: embeddings from offsets == embeddings of gather_windows (incl. the zero-padded tail window)
    monkeypatch.setattr(db, "cosine_affinity", lambda e, use_gpu: asd.cosine_affinity(e, False))
    wav = tmp_path / "m.wav"
    audio_io.write_wav16(wav, conv.wav, conv.sr)
    _, det_g = db.diarize_audio(wav, 0.35, 0.1, 2, 6, return_details=True)
    _, det_c = db.diarize_audio(wav, 0.35, 0.1, 2, 6, return_details=True, encoder=cpu_encode)
    assert np.array_equal(det_g["embeddings"], det_c["embeddings"]) and np.array_equal(det_g["labels"], det_c["labels"])
