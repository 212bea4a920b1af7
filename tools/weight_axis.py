"""Measure, on the GPU, how the engine and the operators behave along the WEIGHT axis, and write profiles/weight_axis.json (the table
README.md quotes; tests/test_gpu_weights.py asserts the same runs against their bars):

  * the forward on the trained-like dicts of tests/helpers/trained_like.py, per geometry, tail, precision and tile choice: cosine
    distance to the float64 oracle at the same weights and inputs next to d_ref32 (the f32 oracle) and d_emu16 (the f32 oracle with
    the engine's f16 stores), their ratio, the bar, the largest activation of the float64 forward, the generator's parameters;
  * relative lengths and packed spans on the exact-f32 engine (the spans also through the uniform engine, one by one);
  * the two operator figures a bar of tests/test_gpu_weights.py is derived from: the column statistics of the MFA layer and the fused
    attention pooling with the dict's asp.conv.

    python tools/weight_axis.py [--out profiles/weight_axis.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import ecapa_plan as P  # noqa: E402
import trained_like as TL  # noqa: E402

PRECISIONS = ("f32", "f32ns", "f32s", "f16")


def lst(a):
    return [float(v) for v in np.asarray(a).reshape(-1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_axis.json"))
    a = ap.parse_args()
    import test_gpu_weights as G
    import wav_lens_ref as WL
    from oracle.ecapa_ref import EcapaRef
    from oracle.fbank_ref import speechbrain_fbank_ref
    from speech_diarization_amd.engine import EmbeddingEngine
    dev = torch.device("cuda", 0)
    nets, forward = {}, []
    for geom, tail, B, n in TL.FORWARD_CASES:
        sd = nets.setdefault((geom, tail), TL.trained_like_state_dict(geom, TL.SEED, tail))
        wav = TL.eval_wav(B, n)
        r64 = TL.oracle64(sd, wav)
        d_ref32, d_emu16 = TL.cos_dist(TL.oracle32(sd, wav), r64), TL.cos_dist(TL.emu16(sd, wav), r64)
        _, inter = EcapaRef(sd, torch.float64).forward_features(torch.from_numpy(speechbrain_fbank_ref(wav)), return_intermediates=True)
        top = max(float(v.abs().max()) for v in inter.values())
        wd = torch.from_numpy(wav).to(dev)
        for precision in PRECISIONS:
            eng = EmbeddingEngine(sd, dev, precision=precision)
            for tiles in P.TILES:
                P.set_tiles(tiles)
                try:
                    got = eng.embed(wd).cpu().numpy()
                finally:
                    P.set_tiles("auto")
                d = TL.cos_dist(got, r64)
                base = d_emu16 if precision == "f16" else d_ref32
                forward.append(dict(geom=geom, tail=tail, B=B, samples=n, precision=precision, tiles=tiles, d_ref32=lst(d_ref32), d_emu16=lst(d_emu16),
                                    distance=lst(d), ratio=float((d / base).max()), bar=lst(TL.bar(precision, d_ref32, d_emu16)), largest_activation=top))
                print(f"{geom:9s} tail {tail} n {n:5d} {precision:6s} {tiles:8s} distance {d.max():.2e}  ratio {(d / base).max():6.2f}")
            del eng
    sd = nets["w128", 2.0]
    eng = EmbeddingEngine(sd, dev)
    wav, lens = TL.lens_wav(3, 32000, G.REL)
    r64 = WL.encode_batch_lens_ref(sd, wav, lens)
    d_ref32 = TL.cos_dist(TL.lens_oracle32(sd, wav, lens), r64)
    d = TL.cos_dist(eng.embed(torch.from_numpy(wav).to(dev), torch.from_numpy(lens).to(dev)).cpu().numpy(), r64)
    lengths = dict(geom="w128", tail=2.0, rel=list(G.REL), d_ref32=lst(d_ref32), distance=lst(d), ratio=float((d / d_ref32).max()))
    signal, starts = TL.span_signal()
    alone = [signal[s: s + n][None] for s, n in zip(starts, TL.SPANS)]
    r64 = np.concatenate([TL.oracle64(sd, w) for w in alone])
    d_ref32 = TL.cos_dist(np.concatenate([TL.oracle32(sd, w) for w in alone]), r64)
    got = eng.embed_spans(torch.from_numpy(signal).to(dev), starts, np.asarray(TL.SPANS)).cpu().numpy()
    one = np.concatenate([eng.embed(torch.from_numpy(w).to(dev)).cpu().numpy() for w in alone])
    net64 = EcapaRef(sd, torch.float64)
    on_hip = np.concatenate([net64.forward_features(eng.features(torch.from_numpy(w).to(dev)).cpu().double()).numpy() for w in alone])
    d = TL.cos_dist(got, r64)
    spans = dict(geom="w128", tail=2.0, spans=list(TL.SPANS), d_ref32=lst(d_ref32), distance=lst(d), ratio=float((d / d_ref32).max()),
                 uniform_engine_on_each_span_alone=lst(TL.cos_dist(one, r64)), packed_against_alone=lst(TL.cos_dist(got, one)),
                 float64_network_on_the_fbank_kernels_features=lst(TL.cos_dist(on_hip, r64)))
    print("lengths", lengths["ratio"], "spans", spans["ratio"], spans["float64_network_on_the_fbank_kernels_features"])
    sd = nets[G.OP_GEOM, 2.0]
    operators = []
    for T, n in sorted(G.OP_T.items()):
        net = G._PointRef(sd)
        net.forward_features(torch.from_numpy(speechbrain_fbank_ref(TL.eval_wav(G.OP_B, n))))
        for dtype in (torch.float32, torch.float16):
            r = G.measure_colstat(dev, sd, net, dtype, T)
            operators.append(dict(op="colstat mfa", dtype=r["dtype"], T=T, mean_err=r["mean_err"], std_err=r["std_err"], bar=2e-5 if r["dtype"] == "f32" else 2e-3,
                                  ratio=max(r["mean_err"], r["std_err"]) / (2e-5 if r["dtype"] == "f32" else 2e-3), constant_pairs=r["constant"],
                                  median_mean_over_std=r["median_mean_over_std"]))
        for mode in ("f32", "split16", "f16"):
            r = G.measure_fused(dev, sd, net, mode, T)
            operators.append(dict(op="fused pooling", mode=mode, T=T, mean_err=float(r["e_mu"].max()), std_err=float(r["e_sd"].max()), bar=2e-5,
                                  ratio=float(r["e_mu"].max()) / 2e-5, logit_width_median=r["width_median"], logit_width_max=r["width_max"], h_max=r["h_max"]))
    for o in operators:
        print(o)
    rec = dict(device="MI355X", generator=dict(TL.PARAMS, seed=TL.SEED),
               forward_note="cosine distance to the float64 oracle per segment; ratio = max over segments of distance / d_ref32 (f16: / d_emu16); "
                            "bar = 16 d + the precision's bar at the init weights", forward=forward, lengths=lengths,
               spans_note="the bar of the spans test is 2 x the ratio recorded here; the last three rows attribute the distance to the fbank features",
               spans=spans, operators_note="geometry w256a128, tail 2.0, B = 3; ratio = error / bar of the operator at the init weights", operators=operators)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
