#!/usr/bin/env python3
"""Record the reference's third entry point, `diar_diag.main`, on scripted inputs -> tests/golden/diar_diag_pipeline.json.

    python -B tests/golden/make_diag_golden.py <path of the reference checkout>

The reference module is imported with doubles, as make_golden.py does: `typer` (command() is the identity, Option / Argument return
their default), inert `soundfile`, `librosa`, `pyloudnorm`, `matplotlib` and `rich`, and scikit-learn's HDBSCAN in the `hdbscan.HDBSCAN`
slot.  Four of its functions are replaced: `load_audio` and `loudness_normalize` hand over a synthetic conversation as it is,
`silero_probs_raw` returns scripted frame probabilities, and `SpeakerEncoder` is `diag_cases.ScriptedEncoder`.  Everything between
them is the reference's own `main` with save_plots=0: its VAD post-processing, context slices, tiling, whitening, clustering,
centres, scores, path, merging and the three writers.

Recorded per case: the arguments, the scripted segments, the piece every `embed` call received (its offset in `y` and its length, or
that it was a tiled copy; stored once per kind of segments and context) and the three files: the csv as text, the json and the srt
as SHA-256 of their bytes.  Also recorded: the reference's VAD helpers on random masks (as run lengths) and signals.  Only inputs and
outputs are written; no reference source is copied."""
import hashlib
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

import diag_cases as DC  # noqa: E402
from make_golden import _Inert, jsonable  # noqa: E402


def import_reference(ref_dir):
    from sklearn.cluster import HDBSCAN
    for n in ("soundfile", "librosa", "librosa.effects", "pyloudnorm", "matplotlib", "matplotlib.pyplot", "rich"):
        sys.modules[n] = _Inert(n)
    sys.modules["rich"].print = lambda *a, **k: None
    ty = types.ModuleType("typer")
    ty.Typer = lambda **k: types.SimpleNamespace(command=lambda *a, **k: (lambda f: f))
    ty.Option = lambda default=None, *a, **k: default
    ty.Argument = lambda default=None, *a, **k: default
    sys.modules["typer"] = ty
    hd = types.ModuleType("hdbscan")
    hd.HDBSCAN = HDBSCAN
    sys.modules["hdbscan"] = hd
    sys.path.insert(0, ref_dir)
    sys.dont_write_bytecode = True
    import diar_diag
    return diar_diag


def bits(m):
    return "".join("1" if v else "0" for v in np.asarray(m).astype(bool))


def record_vad(rdd):
    rng = np.random.default_rng(20260)
    masks = []
    for k in range(200):
        n = int(rng.integers(1, 300))
        m = np.zeros(n, bool)
        pos = int(rng.integers(0, 30))
        while pos < n:
            run = int(rng.integers(1, 90))
            m[pos:pos + run] = True
            pos += run + int(rng.integers(1, 40))
        if k % 4 == 0:
            m[n - int(rng.integers(1, 30)):] = True
        hop_ms = [10.0, 10.0, 12.5, 16.0, 7.5][k % 5]
        min_speech, min_gap = [(250.0, 100.0), (25.0, 5.0), (150.0, 250.0), (0.0, 0.0)][k % 4]
        masks.append(dict(runs=DC.mask_runs(m), hop_ms=hop_ms, min_speech_ms=min_speech, min_gap_ms=min_gap,
                          segments=rdd.mask_to_segments(m, hop_ms, min_speech, min_gap)))
    tracks = []
    for seed in range(4):
        n = [1, 37, 94, 400][seed]
        t = np.arange(n)
        u = np.random.default_rng(seed).random(n)
        probs = np.round(np.clip(0.5 + 0.45 * np.sin(t / (5.0 + seed)) * np.sign(np.sin(t / (31.0 + 3 * seed))) + 0.25 * (u - 0.5), 0, 1), 4)
        probs = probs.astype(np.float32)
        variants = []
        for on, off in [(0.6, 0.4), (0.7, 0.2)]:
            h = rdd.hysteresis_binarize(probs, on, off)
            for open_ms, close_ms in [(80.0, 40.0), (0.0, 40.0), (30.0, 0.0)]:
                variants.append(dict(on=on, off=off, hyst=bits(h), open_ms=open_ms, close_ms=close_ms,
                                     mask=bits(rdd.morph_open_close(h, 10.0, open_ms, close_ms))))
        tracks.append(dict(probs=[round(float(v), 4) for v in probs], variants=variants))      # f32 of the 4-decimal value, as the test reads it
    frames = []
    for n, sr, win_ms, hop_ms in [(100, 16000, 30.0, 10.0), (480, 16000, 30.0, 10.0), (481, 16000, 30.0, 10.0), (16000, 16000, 30.0, 10.0),
                                  (16100, 16000, 25.0, 10.0), (8000, 8000, 30.0, 12.5), (1, 16000, 30.0, 10.0)]:
        y = np.arange(n, dtype=np.float32)
        f, hop = rdd.frame_audio(y, sr, win_ms, hop_ms)
        frames.append(dict(n=n, sr=sr, win_ms=win_ms, hop_ms=hop_ms, shape=list(f.shape), hop=int(hop), first=f[0][:3], last=f[-1][-3:]))
    ctx = []
    y = np.arange(48000, dtype=np.float32)
    for st, ed, c in [(0.0, 0.5, 0.2), (0.1, 0.5, 0.2), (1.0, 2.0, 0.2), (2.9, 3.0, 0.2), (2.5, 3.5, 0.0), (1.2345, 1.9876, 0.2), (0.3333, 0.6667, 0.05)]:
        a = rdd.pad_with_context(y, 16000, st, ed, ctx=c)
        ctx.append(dict(start=st, end=ed, ctx=c, first=int(a[0]), length=int(len(a))))
    return dict(masks=masks, tracks=tracks, frames=frames, context=ctx)


def record_pipeline(rdd):
    conv = DC.conversation()
    y = conv.wav
    n_frames = rdd.frame_audio(y, DC.SR)[0].shape[0]
    rdd.load_audio = lambda path, sr=16000: (y, sr)
    rdd.loudness_normalize = lambda yy, sr, target_lufs=-18.0: yy
    out, pieces = {}, {}
    for name, case in DC.pipeline_cases().items():
        kw = {k: v for k, v in case.items() if k not in ("segs", "rows")}
        segs = DC.scripted_segments(case["segs"], conv.turns, DC.CONVERSATION["duration_s"])
        probs = DC.probs_from_segments(segs, n_frames)
        rdd.silero_probs_raw = lambda yy, sr, win_ms, hop_ms, device="cpu", _p=probs: _p
        spans = []

        class Encoder(DC.ScriptedEncoder):
            def __init__(self, backend=None, device=None, ali_model_id=None):
                super().__init__(DC.scripted_rows(case["rows"], len(segs)))

            def embed(self, a, sr):
                inside = np.shares_memory(a, y)
                spans.append([(a.__array_interface__["data"][0] - y.__array_interface__["data"][0]) // y.itemsize if inside else -1, int(len(a))])
                return super().embed(a, sr)

        rdd.SpeakerEncoder = Encoder
        with tempfile.TemporaryDirectory() as td:
            rdd.main("scripted.wav", out_dir=td, device="cpu", save_plots=0, **kw)
            raw = {k: open(os.path.join(td, f"diarization.{k}"), "rb").read() for k in ("json", "srt", "csv")}
        key = f"{case['segs']}/ctx{kw.get('pad_ctx', 0.2)}"
        assert pieces.setdefault(key, spans) == spans                 # the pieces depend on the segments and the context alone
        out[name] = dict(kwargs=kw, segs=case["segs"], rows=case["rows"], spans=key, csv=raw["csv"].decode("utf-8"),
                         json_sha256=hashlib.sha256(raw["json"]).hexdigest(), srt_sha256=hashlib.sha256(raw["srt"]).hexdigest())
        print(name, len(spans), "pieces,", json.loads(raw["json"])["speakers"])
    return dict(spans=pieces, n_samples=int(len(y)), n_frames=int(n_frames), wav_abs_sum=float(np.abs(y.astype(np.float64)).sum()), cases=out)


def main():
    rdd = import_reference(sys.argv[1])
    payload = dict(vad=record_vad(rdd), pipeline=record_pipeline(rdd))
    path = os.path.join(HERE, "diar_diag_pipeline.json")
    with open(path, "w") as f:
        json.dump(jsonable(payload), f)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
