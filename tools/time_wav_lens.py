#!/usr/bin/env python3
"""Cost of relative lengths (speechbrain's wav_lens): the masked forward against the unmasked one on the SAME padded batch.
HIP-event medians of 5 alternating passes (after one warm-up of each), on the launch stream.
  (a) 10 000 x 2 s segments resident on the device, lengths uniform in [0.5, 1], one forward per pass (the bench step's shape)
  (b) a ragged batch of 32 segments of 0.3 .. 30 s zero-padded to 30 s, as embed_segments pads them, through encode_batch
    python tools/time_wav_lens.py [--precision f32] [--out FILE]   -> one JSON line per case (also appended to FILE)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from speech_diarization_amd import synth
from speech_diarization_amd.engine import EmbeddingEngine
from speech_diarization_amd.speech_encode import HipEcapaEncoder

ap = argparse.ArgumentParser()
ap.add_argument("--precision", default="f32", choices=["f32", "f16", "f32s", "f32ns"])
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
sd = synth.make_ecapa_state_dict(1234)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def compare(name, plain, masked, bar, extra):
    plain(), masked()                                    # warm-up: workspaces, first launches
    torch.cuda.synchronize()
    tp, tm = [], []
    for _ in range(a.passes):
        tp.append(timed(plain))
        tm.append(timed(masked))
    mp, mm = float(np.median(tp)), float(np.median(tm))
    line = {"case": name, "precision": a.precision, "unmasked_ms": round(mp, 3), "masked_ms": round(mm, 3), "ratio": round(mm / mp, 4),
            "bar": bar, "within_bar": mm / mp <= bar, "passes": a.passes, "unmasked_all_ms": [round(x, 3) for x in tp],
            "masked_all_ms": [round(x, 3) for x in tm], **extra}
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


# (a) the bench step's batch, lengths uniform in [0.5, 1]
S, n = 10000, 32000
eng = EmbeddingEngine(sd, dev, max_batch=S, precision=a.precision)
wav = synth.synthetic_segments_device(0, S, n, dev, std=0.1)
g = torch.Generator().manual_seed(0)
rel = (0.5 + 0.5 * torch.rand(S, generator=g)).to(dev)
compare("10000 x 2 s, wav_lens ~ U[0.5, 1]", lambda: eng.embed(wav), lambda: eng.embed(wav, rel_lens=rel), 1.04,
        {"segments": S, "samples": n})
del eng, wav
torch.cuda.empty_cache()

# (b) 32 VAD-like segments of 0.3 .. 30 s zero-padded to the longest
rng = np.random.default_rng(1)
secs = np.exp(rng.uniform(np.log(0.3), np.log(30.0), 32))
secs[0], secs[1] = 30.0, 0.3
n = int(30.0 * 16000)
host = np.zeros((32, n), np.float32)
lens = np.zeros(32, np.float32)
for i, s in enumerate(secs):
    k = int(s * 16000)
    host[i, :k] = synth.synthetic_segments(200 + i, 1, k)[0]
    lens[i] = np.float32(k) / np.float32(n)
enc = HipEcapaEncoder(sd, dev, precision=a.precision)
x = torch.from_numpy(host).to(dev)
wl = torch.from_numpy(lens)
compare("32 ragged segments 0.3 .. 30 s padded to 30 s, encode_batch", lambda: enc.encode_batch(x), lambda: enc.encode_batch(x, wl), 1.05,
        {"segments": 32, "samples": n, "speech_share": round(float(lens.mean()), 4)})
