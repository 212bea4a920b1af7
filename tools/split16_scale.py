"""Measure, on the GPU, how the split operators and the engine behave along the magnitude axis, and write profiles/split16_scale.json
(the table README.md, DESIGN.md and include/sd_hip.h quote; tests/test_gpu_scale.py asserts the same runs against their bars):

  * sd_conv1d_cl_split16, wide and narrow form, with every channel of x at 2^0 .. 2^-12: error against float64, measured and from the
    numpy emulation of the header's arithmetic, absolute and relative to the largest output;
  * the engine in every precision on the quiet / loud twin of the synthetic network (all frame-level activations at c times their
    size) next to c = 1: cosine distance to the float64 oracle on the same state dict.

    python tools/split16_scale.py [--out profiles/split16_scale.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import scale_cases as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split16_scale.json"))
    a = ap.parse_args()
    from oracle import pipeline_ref
    from speech_diarization_amd import synth
    from speech_diarization_amd.engine import EmbeddingEngine
    dev = torch.device("cuda", 0)
    conv = []
    for form in S.ACCURACY_SHAPES:
        for e in S.ACCURACY_EXPONENTS:
            r = S.measure_accuracy(dev, form, e)
            r.update(measured_rel=r["measured"] / r["top"], emulated_rel=r["emulated"] / r["top"], shape=list(S.ACCURACY_SHAPES[form]))
            conv.append(r)
            print(f"{form:6s} x 2^{e:<3d} measured {r['measured_rel']:.2e}  emulated {r['emulated_rel']:.2e}  (of the largest output)")
    sd = synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(128))
    wav = synth.synthetic_segments(0, 3, 16000)
    wd = torch.from_numpy(wav).to(dev)
    engine = []
    for c in (1.0,) + S.ENGINE_SCALES:
        twin = S.scaled_state_dict(sd, c) if c != 1.0 else sd
        ref = pipeline_ref.encode_batch_ref(twin, wav, torch.float64)
        for precision in S.ENGINE_PRECISIONS:
            got = EmbeddingEngine(twin, dev, precision=precision).embed(wd).cpu().numpy()
            cd = float(S.cos_dist(got, ref).max())
            engine.append(dict(log2_c=int(np.log2(c)), precision=precision, cos_dist=cd, bar=1e-3 if precision == "f16" else 1e-5))
            print(f"c = 2^{int(np.log2(c)):<3d} {precision:6s} cosine distance to float64 {cd:.2e}")
    rec = dict(device="MI355X", conv_note="sd_conv1d_cl_split16, every channel of x times 2^log2_scale, no bias; errors are max |y - float64|; "
               "bar = 2 emulated + 2e-6 top", conv=conv,
               engine_note="EcapaConfig.small(128), B = 3, 16000 samples; scale_cases.scaled_state_dict(sd, 2^log2_c) against the float64 oracle on the same dict",
               engine=engine)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
