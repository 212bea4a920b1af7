"""Sweep the AHC cut over the meeting tests/test_gpu_ahc.py diarizes (60 s, 2 voices, the small seeded encoder): for every cosine
threshold the speakers the host route (`clustering="ahc"`) finds and the distance from the cut to the nearest merge height of its
dendrogram.  The pipeline test takes a threshold from this table (2-8 speakers, margin above 1e-3).

    python tools/sweep_ahc_threshold.py [--seconds 60] [--voices 2]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ahc_ref as A  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--voices", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("sweep_ahc_threshold.py embeds on the GPU; there is nothing to sweep without one")
    from speech_diarization_amd import audio_io, cluster, diarization_baseline as db, ecapa_annote, speech_encode, synth
    enc = speech_encode.HipEcapaEncoder(synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(128)), torch.device("cuda", 0))
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = lambda device="cuda": enc
    conv = synth.synthetic_conversation(a.seconds, a.voices, seed=0)
    with tempfile.TemporaryDirectory() as tmp:
        wav = os.path.join(tmp, "meeting.wav")
        audio_io.write_wav16(wav, conv.wav, conv.sr)
        _, det = db.diarize_audio(wav, 0.35, 0.1, 2, 6, clustering="ahc", return_details=True)
    K = det["affinity"]
    for thr in np.round(np.arange(-0.5, 0.951, 0.05), 2):
        labels = cluster.ahc_cosine(K, float(thr))
        print(json.dumps({"windows": int(K.shape[0]), "cos_thr": float(thr), "speakers": int(len(set(labels.tolist()))),
                          "cut_margin": A.cut_margin(K, float(thr))}), flush=True)


if __name__ == "__main__":
    main()
