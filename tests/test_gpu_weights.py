"""Parity along the WEIGHT axis.  Every other GPU module takes its network from `synth.make_ecapa_state_dict` and its operator inputs
from Gaussians; here the engine and the operators see the calibrated, trained-like dicts of tests/helpers/trained_like.py: heavy-tailed
weights, zero rows, negative and 1e-3-sized BatchNorm weights, always-on / always-off channels, attention logits tens wide, saturated
gates, statistics that match the activations.  tests/test_weight_axis_rules.py holds the conditions that make these runs meaningful.

1. The forward in every precision and both tile choices, each run held to its plan, against the float64 oracle at the same weights and
   inputs.  The bar of a run comes from the reference arithmetic at those weights (trained_like.bar), never from the engine.
2. Relative lengths and packed spans on the exact-f32 engine, same bar.
3. The operators at the operating point: inputs are the oracle's intermediates, layers the dict's own."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ecapa_plan as P  # noqa: E402
import trained_like as TL  # noqa: E402
from kernel_selection import CONV_KERNELS, f16_tiles, restore_conv_kernel, select_conv_kernel  # noqa: E402,F401
from launch_log import launches  # noqa: E402

pytestmark = pytest.mark.gpu

PRECISIONS = ("f32", "f32ns", "f32s", "f16")
# routes a case must have taken for its run to count (ecapa_plan.count_mismatches then holds every route to its launches): the split
# modes' narrow, folded, 256x256 and fused forms, the f16 chain
MUST_ROUTE = {
    ("w128", "f32s"): {"split128"}, ("w128", "f16"): {"f16"},
    ("w256a128", "f32s"): {"split128", "asp_fused"}, ("w256a128", "f32ns"): {"asp_fused"}, ("w256a128", "f16"): {"f16", "asp_fused"},
    ("w256a128", "f32"): {"asp_fused", "colstat_finish"},
    ("full", "f32"): {"asp_fused", "colstat_finish"}, ("full", "f32ns"): {"asp_fused", "colstat_finish"},
    ("full", "f16"): {"chain", "f16", "asp_fused", "colstat_finish"},
    ("full", "f32s", "auto"): {"split128_folded", "split256_twin", "asp_fused", "colstat_finish"},
    ("full", "f32s", "wide256"): {"pack", "split256_pack", "split256_twin", "split128", "asp_fused", "colstat_finish"},
}


@pytest.fixture(scope="module")
def nets():
    made = {}

    def get(geom, tail):
        if (geom, tail) not in made:
            made[geom, tail] = TL.trained_like_state_dict(geom, TL.SEED, tail)
        return made[geom, tail]
    return get


@pytest.fixture(scope="module")
def refs(nets):
    """(geom, tail, B, n) -> (wav, float64 embeddings, d_ref32, d_emu16 per segment), computed once and shared by the 8 runs of a case."""
    made = {}

    def get(geom, tail, B, n):
        key = (geom, tail, B, n)
        if key not in made:
            sd, wav = nets(geom, tail), TL.eval_wav(B, n)
            r64 = TL.oracle64(sd, wav)
            made[key] = (wav, r64, TL.cos_dist(TL.oracle32(sd, wav), r64), TL.cos_dist(TL.emu16(sd, wav), r64))
        return made[key]
    return get


@pytest.fixture(scope="module")
def engines(dev, nets):
    from speech_diarization_amd.engine import EmbeddingEngine
    made = {}

    def get(geom, tail, precision):
        if (geom, tail, precision) not in made:
            made[geom, tail, precision] = EmbeddingEngine(nets(geom, tail), dev, precision=precision)
        return made[geom, tail, precision]
    return get


def _planned_run(eng, tiles, plan_args, run):
    """`run()` under the tile choice, with the plan of the same forward and its launch log -> (output, routes)."""
    P.set_tiles(tiles)
    try:
        _, steps = P.read_plan(eng.weights.struct, *plan_args[0], **plan_args[1])
        with launches() as log:
            got = run()
        torch.cuda.synchronize()
    finally:
        P.set_tiles("auto")
    bad = P.count_mismatches(steps, log)
    assert not bad, bad
    return got.cpu().numpy(), {s.route for s in steps}


# ------------------------------------------------------------------ 1. the forward, every precision

@pytest.mark.parametrize("tiles", P.TILES)
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("geom,tail,B,n", TL.FORWARD_CASES, ids=[f"{g}-tail{t:g}-B{B}-n{n}" for g, t, B, n in TL.FORWARD_CASES])
def test_forward_on_trained_like_weights(dev, nets, refs, engines, geom, tail, B, n, precision, tiles):
    """Cosine distance to float64 per segment: f32, f32ns, f32s at most 16 d_ref32 + the precision's bar at the init weights (1e-13,
    f32s 2e-13); f16 at most 16 d_emu16 + 2e-8, d_emu16 from the f32 oracle with the engine's f16 stores (trained_like.EmuF16Ref)."""
    wav, r64, d_ref32, d_emu16 = refs(geom, tail, B, n)
    eng = engines(geom, tail, precision)
    wd = torch.from_numpy(wav).to(dev)
    got, routes = _planned_run(eng, tiles, ((B, P.frames(n)), {}), lambda: eng.embed(wd))
    need = MUST_ROUTE.get((geom, precision, tiles), MUST_ROUTE.get((geom, precision), set()))
    assert need <= routes, (need - routes, routes)
    d, bar = TL.cos_dist(got, r64), TL.bar(precision, d_ref32, d_emu16)
    print(f"\n[{geom} tail {tail} B{B} n{n} {precision} {tiles}] distance {d}, d_ref32 {d_ref32}, d_emu16 {d_emu16}, bar {bar}, "
          f"ratio {(d / (d_emu16 if precision == 'f16' else d_ref32)).max():.2f}")
    assert np.isfinite(got).all()
    assert (d <= bar).all(), (d, bar)


# ------------------------------------------------------------------ 2. segment maps on the exact-f32 engine

REL = (1.0, 0.5, 0.37)
SPANS_RATIO = 26.7          # measured distance / d_ref32 of the packed 32000-sample span: profiles/weight_axis.json, "spans"


@pytest.mark.parametrize("tiles", P.TILES)
def test_relative_lengths_on_trained_like_weights(dev, nets, engines, tiles):
    """speechbrain's wav_lens against the oracle's masked forward (tests/helpers/wav_lens_ref.py, as tests/test_gpu_wav_lens.py)."""
    import wav_lens_ref as WL
    sd = nets("w128", 2.0)
    wav, lens = TL.lens_wav(3, 32000, REL)
    r64 = WL.encode_batch_lens_ref(sd, wav, lens)
    d_ref32 = TL.cos_dist(TL.lens_oracle32(sd, wav, lens), r64)
    eng = engines("w128", 2.0, "f32")
    wd, ld = torch.from_numpy(wav).to(dev), torch.from_numpy(lens).to(dev)
    got, _ = _planned_run(eng, tiles, ((3, P.frames(32000)), dict(map_kind="lengths")), lambda: eng.embed(wd, ld))
    d, bar = TL.cos_dist(got, r64), TL.bar("f32", d_ref32, None)
    print(f"\n[lengths {REL} {tiles}] distance {d}, d_ref32 {d_ref32}, bar {bar}")
    assert np.isfinite(got).all() and (d <= bar).all(), (d, bar)
    assert TL.cos_dist(r64[1:], TL.oracle64(sd, wav)[1:]).min() > 1e-3           # the mask matters: the padded forward is elsewhere


@pytest.mark.parametrize("tiles", P.TILES)
def test_packed_spans_on_trained_like_weights(dev, nets, engines, tiles):
    """Spans of 640, 9600 and 32000 samples in one packed forward against each span embedded alone (float64).

    The bar differs from 16 d_ref32 + 1e-13, by a recorded ratio: the 32000-sample span sits 1.27e-10 from float64, 26.7 times its
    d_ref32 of 4.7e-12 (profiles/weight_axis.json, "spans"), and all of it is the fbank: the FLOAT64 network on the features the
    fbank kernel gives for that span sits 1.24e-10 from float64, on torch's f32 fbank 6e-12; the uniform engine on the span alone
    gives the same 1.4e-10, packed against alone 4e-13.  The fbank kernel holds its own documented bars (1e-3 dB; here 1.3e-4) but
    misses float64 in other bins than torch's f32 STFT does, and these weights are 1000 times more sensitive to features than the
    init.  Hence SPANS_RATIO x 2 in place of 16 (README.md, Weights; include/sd_hip.h at sd_fbank_f32)."""
    sd = nets("w128", 2.0)
    signal, starts = TL.span_signal()
    alone = [signal[s: s + n][None] for s, n in zip(starts, TL.SPANS)]
    r64 = np.concatenate([TL.oracle64(sd, w) for w in alone])
    d_ref32 = TL.cos_dist(np.concatenate([TL.oracle32(sd, w) for w in alone]), r64)
    eng = engines("w128", 2.0, "f32")
    sig = torch.from_numpy(signal).to(dev)
    M = sum(P.frames(n) for n in TL.SPANS)
    got, routes = _planned_run(eng, tiles, ((len(TL.SPANS),), dict(M=M, map_kind="packed")),
                               lambda: eng.embed_spans(sig, starts, np.asarray(TL.SPANS)))
    assert "packed" in routes
    d, bar = TL.cos_dist(got, r64), 2.0 * SPANS_RATIO * d_ref32 + TL.FLOOR["f32"]
    one = np.concatenate([eng.embed(torch.from_numpy(w).to(dev)).cpu().numpy() for w in alone])
    print(f"\n[spans {TL.SPANS} {tiles}] distance {d}, d_ref32 {d_ref32}, bar {bar}; the engine on each span alone: {TL.cos_dist(one, r64)}, "
          f"packed against alone {TL.cos_dist(got, one)}")
    assert TL.cos_dist(got, one).max() <= 16.0 * d_ref32.max() + TL.FLOOR["f32"]        # the packed map itself adds nothing
    assert np.isfinite(got).all() and (d <= bar).all(), (d, bar)


# ------------------------------------------------------------------ 3. the operators at the operating point
# Inputs are the float64 oracle's intermediates on the w256a128 dict (tail 2.0), rounded to f32 once; layers are the dict's own.
# w256a128 because the column statistics need cout % 256 == 0 and the fused pooling 128 attention channels.

OP_GEOM, OP_B = "w256a128", 3
OP_T = {129: 20480, 201: 32000}
F32, F16 = torch.float32, torch.float16


class _PointRef(TL.EcapaRef):
    """float64 `EcapaRef` that keeps what the operator tests feed their kernels: inputs and outputs of named layers."""

    def __init__(self, sd):
        super().__init__(sd, torch.float64)
        self.kept = {}

    def _tdnn(self, x, name, dilation=1):
        y = super()._tdnn(x, name, dilation)
        if name in ("blocks.1.tdnn1", "blocks.2.tdnn1", "blocks.2.res2net_block.blocks.0", "mfa"):
            self.kept[name] = (x, y)
        return y

    def _conv(self, x, name, dilation=1):
        y = super()._conv(x, name, dilation)
        if name in ("asp.conv", "blocks.1.se_block.conv1"):
            self.kept[name] = (x, y)
        return y


def _cl(x):
    """[B, C, T] float64 -> channel-last rows [B T, C], rounded to f32 and held as float64."""
    return x.transpose(1, 2).reshape(-1, x.shape[1]).float().double()


@pytest.fixture(scope="module")
def point(nets):
    from oracle.fbank_ref import speechbrain_fbank_ref
    made = {}

    def get(T):
        if T not in made:
            net = _PointRef(nets(OP_GEOM, 2.0))
            _, inter = net.forward_features(torch.from_numpy(speechbrain_fbank_ref(TL.eval_wav(OP_B, OP_T[T]))), return_intermediates=True)
            made[T] = (net, inter)
        return made[T]
    return get


def _layer(sd, name, fold=False):
    """(w, bias, scale, shift) of a conv + ReLU + BatchNorm layer as f32 arrays: `bn_affine`, and `fold_constant_rows` as the engine packs it."""
    from speech_diarization_amd.engine import bn_affine, fold_constant_rows
    w, b, aff = sd[f"{name}.conv.conv.weight"], sd[f"{name}.conv.conv.bias"], bn_affine(sd, f"{name}.norm.norm")
    if fold:
        b, aff = fold_constant_rows(w, b, aff)
    return w, b, aff[0], aff[1]


def _ref_layer(x, w, b, s, t, T, dil=1):
    """relu(conv(x) + b) s + t in float64 on channel-last rows (reflect padding per segment)."""
    import torch.nn.functional as F
    M, cin = x.shape
    xt = x.view(M // T, T, cin).transpose(1, 2)
    pad = dil * (w.shape[2] - 1) // 2
    if pad:
        xt = F.pad(xt, (pad, pad), mode="reflect")
    y = F.conv1d(xt, torch.from_numpy(w).double(), torch.from_numpy(b).double(), dilation=dil).transpose(1, 2).reshape(M, -1)
    return torch.relu(y) * torch.from_numpy(s).double() + torch.from_numpy(t).double()


def _d(a, dev, dtype=F32):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(dtype).to(dev)


@pytest.mark.parametrize("name", ["blocks.1.tdnn1", "mfa"])
def test_conv_epilogue_with_the_dicts_own_batchnorm_f32(dev, nets, point, name):
    """The layer's real bias, scale and shift (negative, 1e-3-sized, up to 15) on the real block outputs, under every selection of the
    exact-f32 operator: 2e-6 of the largest output against float64, the operator's bar at the init weights.  The sign of gamma is in
    `bn_affine`: a scale taken as |gamma| misses every negated channel by twice its size."""
    from speech_diarization_amd import ops
    sd, T = nets(OP_GEOM, 2.0), 201
    w, b, s, t = _layer(sd, name)
    assert (s < 0).sum() >= len(s) // 12 and (np.abs(s) < 2e-2).sum() >= 1 and np.abs(s).max() > 3.0
    x = _cl(point(T)[0].kept[name][0])
    ref = _ref_layer(x, w, b, s, t, T)
    want64 = _cl(point(T)[0].kept[name][1])
    assert (ref - want64).abs().max() < 1e-4 * want64.abs().max()           # the same layer as the oracle's (its x in f64, ours rounded)
    top = float(ref.abs().max())
    try:
        for sel in CONV_KERNELS:
            select_conv_kernel(sel)
            got = ops.conv1d_cl(_d(x, dev), ops.pack_weight(w, dev), T, cin=w.shape[1], bias=_d(b, dev), act="relu", scale=_d(s, dev), shift=_d(t, dev))
            err = float((got.cpu().double() - ref).abs().max())
            print(f"\n[{name} {sel}] max error {err:.3e}, largest output {top:.2f}, {err / top:.2e} of it")
            assert err <= 2e-6 * max(1.0, top), (sel, err, top)
    finally:
        restore_conv_kernel()


@pytest.mark.parametrize("name", ["blocks.1.tdnn1", "mfa"])
def test_conv_epilogue_with_the_dicts_own_batchnorm_f16_and_split16(dev, nets, point, f16_tiles, name):
    """The same layers on the f16 operator (1e-3 of the largest output, f16-rounded operands in the reference) and on both forms of the
    split operator (2e-6), under both tile choices."""
    from speech_diarization_amd import ops
    sd, T = nets(OP_GEOM, 2.0), 201
    w, b, s, t = _layer(sd, name)
    x = _cl(point(T)[0].kept[name][0])
    kw = dict(cin=w.shape[1], bias=_d(b, dev), act="relu", scale=_d(s, dev), shift=_d(t, dev))
    ref = _ref_layer(x, w, b, s, t, T)
    top = float(ref.abs().max())
    ws, sh = ops.pack_weight_split16(w, dev)
    for form, got in (("wide", ops.conv1d_cl_split16(_d(x, dev), ws, sh, T, **kw)), ("narrow", ops.conv1d_cl_split16(_d(x, dev), ws, sh, T, narrow=True, **kw))):
        err = float((got.cpu().double() - ref).abs().max())
        print(f"\n[{name} split16 {form} {f16_tiles}] max error {err:.3e}, {err / top:.2e} of the largest output")
        assert err <= 2e-6 * max(1.0, top), (form, err, top)
    x16, w16 = x.half().double(), w.astype(np.float16).astype(np.float32)
    ref16 = _ref_layer(x16, w16, b, s, t, T)
    got = ops.conv1d_cl(_d(x, dev, F16), ops.pack_weight(w, dev, F16), T, **kw)
    err = float((got.cpu().double() - ref16).abs().max())
    print(f"\n[{name} f16 {f16_tiles}] max error {err:.3e}, {err / top:.2e} of the largest output")
    assert got.dtype == F16 and err <= 1e-3 * max(1.0, top), (err, top)


def test_conv_epilogue_known_answers(dev, nets, point):
    """A channel whose scale is exactly 0 stores its shift bit for bit on every row; a row without weights stores relu(bias) scale +
    shift bit for bit (as one fused multiply-add or as two roundings: either is the epilogue's statement)."""
    from speech_diarization_amd import ops
    sd, T = nets(OP_GEOM, 2.0), 201
    w, b, s, t = _layer(sd, "mfa")
    s = s.copy()
    s[::7] = 0.0
    dead = ~np.any(w.reshape(w.shape[0], -1) != 0, axis=1)
    assert dead.sum() >= 2 and (b[dead] > 0).any()
    x = _cl(point(T)[0].kept["mfa"][0])
    fused = (np.maximum(b, 0).astype(np.float64) * s + t).astype(np.float32)
    two = (np.maximum(b, 0) * s).astype(np.float32) + t
    try:
        for sel in CONV_KERNELS:
            select_conv_kernel(sel)
            got = ops.conv1d_cl(_d(x, dev), ops.pack_weight(w, dev), T, cin=w.shape[1], bias=_d(b, dev), act="relu", scale=_d(s, dev), shift=_d(t, dev)).cpu().numpy()
            assert np.array_equal(got[:, ::7], np.broadcast_to(t[::7], got[:, ::7].shape)), sel
            rows = got[:, dead]
            assert (rows == rows[0]).all() and ((rows[0] == fused[dead]) | (rows[0] == two[dead])).all(), sel
    finally:
        restore_conv_kernel()


COLSTAT_STD_RATIO = 2.25      # f32 std error 4.5e-5 against the 2e-5 bar: profiles/weight_axis.json, "operators"


def measure_colstat(dev, sd, net, dtype, T):
    """The MFA layer as the engine packs it with column statistics about pivot = shift -> the errors against mean / std of the stored
    output over the live channels, and what the exactly constant channels give."""
    from speech_diarization_amd import ops
    w, b, s, t = _layer(sd, "mfa", fold=True)
    x = _cl(net.kept["mfa"][0])
    M, cout = x.shape[0], w.shape[0]
    # constant in exact arithmetic on the operands the kernel sees (always off behind the ReLU, or no weights): the stored f16 output
    # can look constant where the f32 values the statistics are taken from are not
    xr, wr = (x.half().double(), w.astype(np.float16).astype(np.float32)) if dtype == F16 else (x, w)
    ref = _ref_layer(xr, wr, b, s, t, T).view(OP_B, T, cout)
    const = ref.max(1).values == ref.min(1).values
    cs = torch.full((ops.colstat_floats(M, cout),), float("nan"), device=dev)
    y = ops.conv1d_cl(_d(x, dev, dtype), ops.pack_weight(w, dev, dtype), T, cin=w.shape[1], bias=_d(b, dev), act="relu", scale=_d(s, dev),
                      shift=_d(t, dev), colstat=cs)
    st = ops.colstat_finish(cs, y, OP_B, T, pivot=_d(t, dev), want_std=True).cpu().double()
    yd = y.cpu().double().view(OP_B, T, cout)
    mean, std = yd.mean(1), yd.std(1, unbiased=False)
    about = ((mean - torch.from_numpy(t).double()).abs() / std.clamp_min(1e-30))[~const]
    return dict(dtype="f16" if dtype == F16 else "f32", T=T, mean_err=float((st[:, :cout] - mean)[~const].abs().max()),
                std_err=float((st[:, cout:] - std)[~const].abs().max()), constant=int(const.sum()), constant_channels=int(const.all(0).sum()),
                median_mean_over_std=float(about.median()), const_mean=st[:, :cout][const], const_std=st[:, cout:][const], const_stored=yd[:, 0][const])


@pytest.mark.parametrize("T", sorted(OP_T))
@pytest.mark.parametrize("dtype", [F32, F16], ids=["f32", "f16"])
def test_column_statistics_of_the_mfa_layer(dev, nets, point, dtype, T):
    """The MFA layer as the engine packs it (`fold_constant_rows`), column statistics about pivot = shift, against mean and std of the
    STORED output.  The live channels have |mean - pivot| / std of about 1.  The exactly constant channels -- always off behind the
    ReLU, or without weights -- give the stored value and sqrt(eps): that is the clamp, and without the fold a row without weights
    and with a positive bias gives 3e-4 of its constant instead.

    Bars: the operators' 2e-5 (f16: 2e-3), except the f32 std, which measured 4.5e-5 (T = 129) and 3.9e-5 (T = 201) on this layer:
    COLSTAT_STD_RATIO = 2.25 times the bar, recorded in profiles/weight_axis.json ("operators").  It is the documented cancellation
    of the one-pass form about the pivot (include/sd_hip.h, sd_colstat_finish_dt) on the always-on channels (bias + 3: the mean about
    the pivot several times the std), which this issue leaves unbounded; the bar is twice the recorded ratio."""
    r = measure_colstat(dev, nets(OP_GEOM, 2.0), point(T)[0], dtype, T)
    print(f"\n[mfa colstat {r['dtype']} T={T}] mean error {r['mean_err']:.2e}, std error {r['std_err']:.2e}, {r['constant']} constant (segment, "
          f"channel) pairs, median |mean - pivot| / std {r['median_mean_over_std']:.2f}")
    tol = 2e-5 if dtype == F32 else 2e-3
    assert r["mean_err"] <= tol and r["std_err"] <= (2.0 * COLSTAT_STD_RATIO * tol if dtype == F32 else tol)
    assert r["constant_channels"] >= 10 and 0.3 < r["median_mean_over_std"] < 3.0
    if dtype == F32:
        assert torch.equal(r["const_mean"], r["const_stored"])
    else:
        assert (r["const_mean"] - r["const_stored"]).abs().max() <= tol
    torch.testing.assert_close(r["const_std"], torch.full_like(r["const_std"], 1e-6), rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("name,narrow,dil", [("blocks.2.tdnn1", False, 1), ("blocks.2.res2net_block.blocks.0", True, 3)])
def test_split_convs_with_heavy_tailed_weights(dev, nets, point, f16_tiles, name, narrow, dil):
    """The rule of tools/split16_scale.py on the dict's weights: the error against float64 within twice the error of the numpy
    emulation of hi hi + hi lo + lo hi (exact_cases.split16_conv_sum) plus 2e-6 of the largest output."""
    import exact_cases as E
    import scale_cases as S
    from speech_diarization_amd import ops
    sd, T = nets(OP_GEOM, 2.0), 201
    w = sd[f"{name}.conv.conv.weight"]
    x = _cl(point(T)[0].kept[name][0]).numpy()
    src = E.source_rows((T,) * OP_B, w.shape[2], dil)
    ref, emul = E.conv_sum(x, w.astype(np.float64), src), E.split16_conv_sum(x, w.astype(np.float64), src)
    e_emul, bar = S.accuracy_bar(ref, emul)
    ws, sh = ops.pack_weight_split16(w, dev)
    got = ops.conv1d_cl_split16(_d(x, dev), ws, sh, T, cin=w.shape[1], dil=dil, narrow=narrow)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max())
    print(f"\n[{name} {f16_tiles}] error {err:.3e}, emulation {e_emul:.3e}, bar {bar:.3e}, largest output {np.abs(ref).max():.2f}")
    assert err <= bar, (err, bar)


def _pool_ref(a1, wc, h, B, T):
    Cc = h.shape[1]
    a = torch.softmax((a1 @ wc.T).view(B, T, Cc), dim=1)
    hr = h.view(B, T, Cc)
    mu = (a * hr).sum(1)
    return mu, torch.sqrt((a * (hr - mu[:, None]) ** 2).sum(1).clamp_min(1e-12)), (a1 @ wc.T).view(B, T, Cc)


FUSED_MEAN_RATIO = 1.42       # mean error 2.84e-5 (split form, T = 129) against the 2e-5 bar: profiles/weight_axis.json, "operators"


def measure_fused(dev, sd, net, mode, T):
    from speech_diarization_amd import ops
    wc = torch.from_numpy(sd["asp.conv.conv.weight"][:, :, 0]).double()
    a1, h = _cl(net.kept["asp.conv"][0]), _cl(net.kept["mfa"][1])
    Cc = h.shape[1]
    if mode == "f16":
        a1, h, wc = a1.half().double(), h.half().double(), wc.half().double()
    g = 1.0
    while mode == "split16" and float(wc.abs().max()) / g >= 256.0:
        g *= 2.0
    mu, sd_, logits = _pool_ref(a1, wc, h, OP_B, T)
    width = (logits.max(1).values - logits.min(1).values)
    dt = F16 if mode == "f16" else F32
    got = ops.asp_attend_pool(_d(a1 * g, dev, dt), ops.pack_weight((wc / g)[:, :, None].float(), dev, dt), _d(h, dev, dt), OP_B, T,
                              split16=mode == "split16").cpu().double()
    return dict(mode=mode, T=T, got=got, mu=mu, sd=sd_, e_mu=(got[:, :Cc] - mu).abs(), e_sd=(got[:, Cc:] - sd_).abs(),
                width_median=float(width.median()), width_max=float(width.max()), h_max=float(h.abs().max()))


@pytest.mark.parametrize("T", sorted(OP_T))
@pytest.mark.parametrize("mode", ["f32", "split16", "f16"])
def test_fused_attention_pooling_with_the_dicts_asp_conv(dev, nets, point, mode, T):
    """a1 and h from the oracle, asp.conv from the dict: logits tens wide (the widest 400), constant h channels, |h| up to 20.  f16:
    the mean to 2e-5 max(1, |mean|) and the std to the bound of test_fused_f16_pooling_bounds_the_cancellation with each channel's own
    mean and sd.  The stand-alone split entry scales its weights by a fixed 2^8 and clamps from |w| = 256 on
    (test_split16_attention_logits_with_large_weights), so the power of two that brings max |w| under 256 moves onto a1, exactly;
    the layer's own 2^s is the forward's (section 1).

    f32 and split: the std holds the 2e-5 of test_fused_attention_pooling_matches_f64 / ..._split16_...; the mean measured 1.2e-5 /
    2.0e-5 (f32, T = 129 / 201) and 2.8e-5 / 8e-6 (split): FUSED_MEAN_RATIO = 1.42 times that bar, recorded in
    profiles/weight_axis.json ("operators").  Those tests weigh h of 1.5 with logits of +-1; here a logit is a sum of 128 products of up
    to 296, so its f32 rounding alone moves a weight by 1e-5 of itself, and |h - mean| is up to 20.  Both forms miss alike, so it is no
    property of the split product; the bar is twice the recorded ratio."""
    r = measure_fused(dev, nets(OP_GEOM, 2.0), point(T)[0], mode, T)
    print(f"\n[fused pooling {mode} T={T}] mean error {float(r['e_mu'].max()):.2e}, std error {float(r['e_sd'].max()):.2e}; logit width median "
          f"{r['width_median']:.1f}, max {r['width_max']:.0f}; max |h| {r['h_max']:.1f}")
    assert r["width_median"] > 5.0 and r["width_max"] > 50.0
    assert bool(torch.isfinite(r["got"]).all())
    if mode == "f16":
        assert (r["e_mu"] <= 2e-5 * r["mu"].abs().clamp_min(1.0)).all()
        assert (r["e_sd"] <= r["mu"] * r["mu"] * 2.0 ** -21 / (2.0 * r["sd"]) + 2e-4).all()
    else:
        assert float(r["e_mu"].max()) <= 2.0 * FUSED_MEAN_RATIO * 2e-5 and float(r["e_sd"].max()) < 2e-5


def test_saturated_se_gates(dev, nets, point):
    """The dict's SE pair on segment means scaled until the pre-sigmoid values reach 40 at both ends: the per-segment GEMMs within 1e-6 of float64,
    the gate exactly 1 where sigmoid is 1 in f32 (z > 17.5: 1 - 2^-25 rounds up) and never outside [0, 1]; `se_scale_residual` on the
    block's real tensors within 1e-6 max(1, |y|) -- beyond |y| = 16 half an f32 ulp is already 1e-6."""
    from speech_diarization_amd import ops
    sd, T = nets(OP_GEOM, 2.0), 201
    net, inter = point(T)
    w1, b1 = sd["blocks.1.se_block.conv1.conv.weight"], sd["blocks.1.se_block.conv1.conv.bias"]
    w2, b2 = sd["blocks.1.se_block.conv2.conv.weight"], sd["blocks.1.se_block.conv2.conv.bias"]
    m = net.kept["blocks.1.se_block.conv1"][0][:, :, 0].float().double()          # [B, C]: the squeeze of block 1

    def pre(c):
        z1 = torch.relu((m * c) @ torch.from_numpy(w1[:, :, 0]).double().T + torch.from_numpy(b1).double())
        return z1, z1.float().double() @ torch.from_numpy(w2[:, :, 0]).double().T + torch.from_numpy(b2).double()
    c = 1.0
    for _ in range(20):
        z = pre(c)[1]
        c *= 40.0 / min(float(z.max()), -float(z.min()))          # both ends reach 40
    mc = (m * c).float().double()
    z1 = torch.relu(mc @ torch.from_numpy(w1[:, :, 0]).double().T + torch.from_numpy(b1).double())
    assert 35.0 < min(float(pre(c)[1].max()), -float(pre(c)[1].min())) < 45.0
    h1 = ops.seg_gemm(_d(mc, dev), ops.pack_weight(w1, dev), cin=w1.shape[1], bias=_d(b1, dev), act="relu")
    assert float((h1.cpu().double() - z1).abs().max()) <= 1e-6 * max(1.0, float(z1.abs().max()))
    z = h1.cpu().double() @ torch.from_numpy(w2[:, :, 0]).double().T + torch.from_numpy(b2).double()
    gate = ops.seg_gemm(h1, ops.pack_weight(w2, dev), cin=w2.shape[1], bias=_d(b2, dev), act="sigmoid")
    g = gate.cpu().double()
    print(f"\n[gates] c = {c:.3g}, pre-sigmoid range [{float(z.min()):.1f}, {float(z.max()):.1f}], gate error {float((g - torch.sigmoid(z)).abs().max()):.2e}, "
          f"{int((z > 17.5).sum())} gates at 1, {int((z < -17.5).sum())} below 3e-8")
    assert float((g - torch.sigmoid(z)).abs().max()) <= 1e-6
    assert (z > 17.5).sum() > 0 and (z < -17.5).sum() > 0
    assert bool((g[z > 17.5] == 1.0).all()) and bool((g >= 0).all()) and bool((g <= 1.0).all()) and bool((g[z < -17.5] < 3e-8).all())
    x, res = _cl(net.kept["blocks.1.tdnn1"][0]), _cl(inter["block1"])          # real tensors of the block's width
    y = ops.se_scale_residual(_d(x, dev), gate, _d(res, dev), OP_B, T).cpu().double()
    want = g.repeat_interleave(T, 0) * x + res
    assert ((y - want).abs() <= 1e-6 * want.abs().clamp_min(1.0)).all()
