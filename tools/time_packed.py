#!/usr/bin/env python3
"""Packed spans against the ways segments of different lengths are embedded without them (exact f32).  HIP-event medians of 5
alternating passes after one warm-up of each, on the launch stream; the results of both sides are compared in the same run.
  (a) 32 VAD-like segments of 0.3 .. 30 s: zero-padded to 30 s through encode_batch (time_wav_lens case b) against encode_spans
  (b) 1 500 VAD-like segments of 0.3 .. 20 s of one recording: embed_segments (batches of 32, padded) against embed_segments(packed=True)
  (c) 200 segments: a loop of B = 1 encode_batch calls (the reference's diagnostic pattern) against one encode_spans
    python tools/time_packed.py [--out FILE]   -> one JSON line per case (also appended to FILE)"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from speech_diarization_amd import anti_stick_diarize as A
from speech_diarization_amd import speech_encode, synth
from speech_diarization_amd.speech_encode import HipEcapaEncoder

ap = argparse.ArgumentParser()
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
sd = synth.make_ecapa_state_dict(1234)
enc = HipEcapaEncoder(sd, dev)
speech_encode.using_ecapa_encoder = lambda *args, **kw: enc       # the pipeline's encoder is this one


def cos_dist(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return 1.0 - (x * y).sum(1) / (np.linalg.norm(x, axis=1) * np.linalg.norm(y, axis=1))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def compare(name, base_name, base, packed, extra, same=None):
    rb, rp = base(), packed()                                      # warm-up: workspaces, first launches
    torch.cuda.synchronize()
    tb, tp = [], []
    for _ in range(a.passes):
        tb.append(timed(base)[0])
        tp.append(timed(packed)[0])
    mb, mp = float(np.median(tb)), float(np.median(tp))
    line = {"case": name, "baseline": base_name, "baseline_ms": round(mb, 3), "packed_ms": round(mp, 3), "speedup": round(mb / mp, 3),
            "passes": a.passes, "baseline_all_ms": [round(x, 3) for x in tb], "packed_all_ms": [round(x, 3) for x in tp], **extra}
    if same is not None:
        line.update(same(rb, rp))
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


def vad_like(seed, count, hi):
    rng = np.random.default_rng(seed)
    secs = np.exp(rng.uniform(np.log(0.3), np.log(hi), count))
    secs[0], secs[1] = hi, 0.3
    return (secs * 16000).astype(np.int64)


# (a) 32 segments of 0.3 .. 30 s (time_wav_lens.py's case b): padded to the longest against packed spans of one signal
lens = vad_like(1, 32, 30.0)
n = int(lens.max())
host = np.zeros((32, n), np.float32)
for i, k in enumerate(lens):
    host[i, :k] = synth.synthetic_segments(200 + i, 1, int(k))[0]
x = torch.from_numpy(host).to(dev)
sig = torch.from_numpy(np.concatenate([host[i, :k] for i, k in enumerate(lens)])).to(dev)
starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
compare("32 segments 0.3 .. 30 s", "encode_batch padded to 30 s", lambda: enc.encode_batch(x).squeeze(1),
        lambda: enc.encode_spans(sig, starts, lens, to_host=False),
        {"segments": 32, "speech_share": round(float(lens.sum() / (32 * n)), 4), "frames_padded": int(32 * (1 + n // 160)),
         "frames_packed": int((1 + lens // 160).sum())})
del x, sig
torch.cuda.empty_cache()

# (b) a meeting's worth of VAD-like segments: the pipeline's embed_segments, padded batches of 32 against packed spans
lens = vad_like(2, 1500, 20.0)
total = int(lens.sum() + 16000 * 60)
y = synth.synthetic_segments(3, 1, total)[0]
rng = np.random.default_rng(4)
st_s = np.sort(rng.integers(0, total - lens.max(), lens.size))
segs = [A.Segment(float(s) / 16000, float(s + k) / 16000) for s, k in zip(st_s, lens)]
compare("1500 segments 0.3 .. 20 s, embed_segments", "embed_segments (batches of 32, padded)", lambda: A.embed_segments(y, 16000, segs),
        lambda: A.embed_segments(y, 16000, segs, packed=True), {"segments": len(segs), "audio_s": round(float(lens.sum()) / 16000, 1)})

# (c) 200 segments: one B = 1 call per segment against one encode_spans call, same results within f32 rounding
lens = vad_like(5, 200, 20.0)
total = int(lens.sum())
y = synth.synthetic_segments(6, 1, total)[0]
starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
yd = torch.from_numpy(y).to(dev)
pieces = [yd[s:s + k][None] for s, k in zip(starts, lens)]
compare("200 segments 0.3 .. 20 s", "loop of encode_batch(B = 1)", lambda: torch.cat([enc.encode_batch(p).squeeze(1) for p in pieces]).cpu().numpy(),
        lambda: enc.encode_spans(yd, starts, lens), {"segments": 200},
        same=lambda rb, rp: {"max_cos_loop_vs_packed": float(cos_dist(rb, rp).max())})
