"""The f16-operand / f32-accumulate path (BASELINE.json configs[4]) against the float64 oracle.

Operands are rounded to f16 (11-bit significand, the precision of the TF32 matmuls the reference
enables on its CUDA path), sums are f32.  The bar is north_star's: embeddings within 1e-3 cosine of
the reference CPU path and identical cluster assignments; the per-operator bound is the f16
rounding of inputs and outputs (2^-11 relative)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from launch_log import expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["wide256", "auto"], autouse=True)
def f16_kernel_choice(request):
    """"wide256" pins the 256x256 kernel for every cout >= 1024 layer (the small shapes of this file would otherwise take the
    128x128 kernel: launches of at most 128 big tiles do since round 3); "auto" is the shipped selection."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    N.check(lib.sd_set_tuning(N.SD_TUNE_F16_NARROW_TILES, 0 if request.param == "wide256" else -1), "sd_set_tuning")
    yield request.param
    N.check(lib.sd_set_tuning(N.SD_TUNE_F16_NARROW_TILES, -1), "sd_set_tuning")


def _cos_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def _ref_conv_cl(x, w, b, T, dil):
    M, cin = x.shape
    xt = x.view(M // T, T, cin).transpose(1, 2)
    pad = dil * (w.shape[2] - 1) // 2
    if pad:
        xt = F.pad(xt, (pad, pad), mode="reflect")
    return F.conv1d(xt, w, b, dilation=dil).transpose(1, 2).reshape(M, -1)


@pytest.mark.parametrize("B,T,cin,cout,k,dil,xdt,ydt", [
    (3, 201, 1024, 1024, 1, 1, torch.float16, torch.float16),
    (5, 101, 128, 128, 3, 3, torch.float16, torch.float16),
    (2, 201, 80, 256, 5, 1, torch.float32, torch.float16),     # stem: f32 features in, f16 out, cin % 64 != 0
    (4, 33, 128, 3072, 1, 1, torch.float16, torch.float32),    # attention logits stay f32
    (3, 50, 256, 200, 1, 1, torch.float16, torch.float16),     # cout not a multiple of the tile
])
def test_conv1d_cl_f16_matches_f64(dev, B, T, cin, cout, k, dil, xdt, ydt):
    from speech_diarization_amd import ops
    g = torch.Generator().manual_seed(B * 77 + T)
    x = torch.randn(B * T, cin, generator=g)
    w = torch.randn(cout, cin, k, generator=g) / np.sqrt(cin * k)
    b = torch.randn(cout, generator=g)
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g)
    xq = x.to(xdt)
    wq = w.half()
    # reference on the SAME rounded operands, float64 arithmetic: isolates accumulation + output rounding
    ref = torch.relu(_ref_conv_cl(xq.double(), wq.double(), b.double(), T, dil)) * scale.double() + shift.double()
    got = ops.conv1d_cl(xq.to(dev), ops.pack_weight(w, dev, torch.float16), T, cin=cin, dil=dil, bias=b.to(dev), act="relu",
                        scale=scale.to(dev), shift=shift.to(dev), out_dtype=ydt)
    torch.cuda.synchronize()
    assert got.dtype == ydt
    tol = (1e-3 if ydt == torch.float16 else 2e-5) * max(1.0, ref.abs().max().item())
    assert (got.cpu().double() - ref).abs().max().item() < tol


def test_conv1d_cl_f16_tee(dev):
    from speech_diarization_amd import ops
    g = torch.Generator().manual_seed(9)
    B, T, C, hid = 3, 57, 256, 64
    xbig = torch.randn(B * T, C, generator=g).half()
    w = (torch.randn(hid, hid, 3, generator=g) / 14).half()
    x_d = xbig.to(dev)
    out = torch.zeros(B * T, C, device=dev, dtype=torch.float16)
    tee = torch.zeros(B * T, hid, device=dev, dtype=torch.float16)
    ops.conv1d_cl(x_d, ops.pack_weight(w.float(), dev, torch.float16), T, cin=hid, dil=2, act="relu", a_col0=64, out=out, o_col0=64,
                  tee=tee, tee_lo=0, tee_hi=hid, tee_add=x_d, ta_col0=128)
    torch.cuda.synchronize()
    y = torch.relu(_ref_conv_cl(xbig[:, 64:128].double().contiguous(), w.double(), None, T, 2))
    assert (out[:, 64:128].cpu().double() - y).abs().max() < 2e-3
    assert out[:, :64].abs().max() == 0 and out[:, 128:].abs().max() == 0
    assert (tee.cpu().double() - (y + xbig[:, 128:192].double())).abs().max() < 4e-3


def test_conv1d_cl_f16_wide_output_with_plain_tee(dev):
    """cout >= 1024 runs on the 256x256 kernel, whose epilogue carries the store-only tee (tdnn1 -> first Res2Net input)."""
    from speech_diarization_amd import ops
    g = torch.Generator().manual_seed(21)
    B, T, cin, cout, chunk = 3, 201, 256, 1024, 128
    x = torch.randn(B * T, cin, generator=g).half()
    w = (torch.randn(cout, cin, 1, generator=g) / 16).half()
    bias = torch.randn(cout, generator=g)
    tee = torch.zeros(B * T, chunk, device=dev, dtype=torch.float16)
    out = ops.conv1d_cl(x.to(dev), ops.pack_weight(w.float(), dev, torch.float16), T, cin=cin, bias=bias.to(dev), act="relu",
                        tee=tee, tee_lo=chunk, tee_hi=2 * chunk, out_dtype=torch.float16)
    torch.cuda.synchronize()
    ref = torch.relu(_ref_conv_cl(x.double(), w.double(), bias.double(), T, 1))
    assert (out.cpu().double() - ref).abs().max() < 1e-3 * max(1.0, ref.abs().max().item())
    assert torch.equal(tee, out[:, chunk:2 * chunk])


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("B,T,Cc", [(3, 201, 512), (2, 101, 256), (4, 33, 256), (2, 256, 256), (5, 1, 256), (2, 64, 768), (1, 129, 3072), (2, 208, 1024),
                                    (2, 150, 256), (2, 192, 256), (2, 193, 512), (2, 65, 256), (3, 16, 256), (2, 17, 256), (2, 240, 256)])
def test_fused_attention_pooling_matches_f64(dev, B, T, Cc, dtype):
    """asp.conv + softmax over T + weighted mean/std in one kernel vs float64 on the same operands,
    and vs the two-operator path it replaces (which stores the logits in the activation dtype)."""
    import ctypes as C
    from speech_diarization_amd import _native as N
    from speech_diarization_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + T)
    att = 128
    a1 = torch.tanh(torch.randn(B * T, att, generator=g)).to(dtype)
    wc = (torch.randn(Cc, att, 1, generator=g) / 4).to(dtype)
    h = (torch.randn(B * T, Cc, generator=g) * 1.5 + 0.3).to(dtype)
    assert ops.asp_attend_pool_supported(dtype, T, Cc, att)
    wp = ops.pack_weight(wc.float(), dev, dtype)
    a1_d, h_d = a1.to(dev), h.to(dev)
    got = ops.asp_attend_pool(a1_d, wp, h_d, B, T).cpu().double()
    logits = (a1.double() @ wc[:, :, 0].double().T).view(B, T, Cc)
    a = torch.softmax(logits, dim=1)
    hr = h.double().view(B, T, Cc)
    mu = (a * hr).sum(1)
    sd = torch.sqrt(((a * (hr - mu[:, None]) ** 2).sum(1)).clamp_min(1e-12))
    assert (got[:, :Cc] - mu).abs().max() < 2e-5
    if T > 1:
        assert (got[:, Cc:] - sd).abs().max() < (2e-4 if dtype == torch.float16 else 2e-5)
    else:
        assert got[:, Cc:].abs().max() < 2e-3          # one frame: sd = sqrt(clamp(0)) up to f32 cancellation
    e = ops.conv1d_cl(a1_d, wp, T, cin=att, out_dtype=dtype)
    two = torch.empty(B, 2 * Cc, device=dev)
    N.check(N.load().sd_asp_pool_dt(e.data_ptr(), Cc, h_d.data_ptr(), N.SD_DT_F16 if dtype == torch.float16 else N.SD_DT_F32, Cc, B, T, Cc,
                                    C.c_float(1e-12), two.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "asp")
    assert (got[:, :Cc] - two[:, :Cc].cpu().double()).abs().max() < (2e-2 if dtype == torch.float16 else 2e-5)


@pytest.mark.parametrize("B,T,cin,cout", [(3, 150, 64, 1024), (7, 301, 128, 1024), (5, 201, 96, 2048)])
def test_wide_f32_kernel_column_statistics(dev, B, T, cin, cout):
    """The 256x256 f32 ring kernel (large launches of the wide layers) behind the same statistics contract; pinned here by the
    tuning knob because test-sized launches would never select it."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    N.check(lib.sd_set_tuning(N.SD_TUNE_WIDE_TILES, 0), "sd_set_tuning")
    try:
        test_epilogue_column_statistics(dev, torch.float32, B, T, cin, cout)
    finally:
        N.check(lib.sd_set_tuning(N.SD_TUNE_WIDE_TILES, -1), "sd_set_tuning")


def test_fused_attention_pooling_refuses_what_it_does_not_cover(dev):
    from speech_diarization_amd import ops
    assert not ops.asp_attend_pool_supported(torch.float16, 300, 256, 128)
    assert not ops.asp_attend_pool_supported(torch.float16, 100, 384, 128)
    assert not ops.asp_attend_pool_supported(torch.float32, 100, 256, 64)
    with pytest.raises(RuntimeError, match="not covered"):
        ops.asp_attend_pool(torch.zeros(300, 128, device=dev, dtype=torch.float16), torch.zeros(256, 1, 128, device=dev, dtype=torch.float16),
                            torch.zeros(300, 256, device=dev, dtype=torch.float16), 1, 300)


@pytest.mark.parametrize("wdt,B,T,cin,cout", [
    (torch.float32, 5, 201, 64, 256),      # f32 kernel, partial last tile (1005 rows)
    (torch.float32, 4, 128, 32, 512),      # tiles aligned with segments
    (torch.float16, 5, 201, 64, 256),      # register-staged f16 kernel
    (torch.float16, 3, 150, 64, 1024),     # 256x256 f16 kernel (two 128-row halves per tile)
    (torch.float16, 7, 301, 128, 1024),    # last 256-row tile: second half starts past the last row
    (torch.float16, 3, 201, 64, 1024),
    (torch.float32, 9, 101, 64, 256),      # 1 s windows: a 128-row tile spans three segments
    (torch.float32, 13, 64, 32, 256),      # shortest supported segments
    (torch.float16, 9, 101, 64, 256),
    (torch.float16, 11, 101, 64, 1024),    # wide output with T < 128: the 128x128 kernel takes it (three parts)
])
def test_epilogue_column_statistics(dev, wdt, B, T, cin, cout):
    """SE squeeze mean / global mean+std straight from the conv epilogue == statistics of the stored output."""
    from speech_diarization_amd import ops
    g = torch.Generator().manual_seed(T * 7 + cout)
    M = B * T
    x = torch.randn(M, cin, generator=g).to(wdt)
    w = torch.randn(cout, cin, 1, generator=g) / np.sqrt(cin)
    bias, scale, shift = torch.randn(cout, generator=g), torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 2
    n_cs = ops.colstat_floats(M, cout)
    cs = torch.full((n_cs + 8192,), float("nan"), device=dev)          # guard words behind the buffer
    y = ops.conv1d_cl(x.to(dev), ops.pack_weight(w, dev, wdt), T, cin=cin, bias=bias.to(dev), act="relu", scale=scale.to(dev),
                      shift=shift.to(dev), colstat=cs)
    y_plain = ops.conv1d_cl(x.to(dev), ops.pack_weight(w, dev, wdt), T, cin=cin, bias=bias.to(dev), act="relu", scale=scale.to(dev),
                            shift=shift.to(dev))
    # the stored output does not change (to rounding: without colstat a launch this small takes the 32x32 split-K kernel)
    assert (y.float() - y_plain.float()).abs().max() <= 2e-3 * y_plain.float().abs().max() * (1.0 if wdt == torch.float16 else 1e-3)
    units = cs[:n_cs].view(-1, 6, cout)           # [sum part 0..2 | sum of squares part 0..2]; part 2 only exists for T < 128
    assert bool(torch.isfinite(units[:, [0, 1, 3, 4]]).all()) and bool(torch.isnan(cs[n_cs:]).all())   # every tile wrote, nobody wrote past the end
    if T < 128:
        assert bool(torch.isfinite(units).all())
    st = ops.colstat_finish(cs, y, B, T, pivot=shift.to(dev), want_std=True).cpu().double()
    mean_only = ops.colstat_finish(cs, y, B, T, pivot=shift.to(dev)).cpu().double()
    yr = y.cpu().double().view(B, T, cout)
    tol = 2e-5 if wdt == torch.float32 else 2e-3                     # f16: statistics of the UNROUNDED outputs vs the rounded store
    assert (st[:, :cout] - yr.mean(1)).abs().max() < tol
    assert (st[:, cout:] - yr.std(1, unbiased=False)).abs().max() < tol
    assert torch.equal(mean_only, st[:, :cout])


def test_epilogue_column_statistics_refuses_short_segments(dev):
    from speech_diarization_amd import ops
    x = torch.zeros(5 * 50, 64, device=dev)
    w = ops.pack_weight(torch.zeros(256, 64, 1), dev)
    with pytest.raises(RuntimeError, match="colstat needs"):
        ops.conv1d_cl(x, w, 50, cin=64, act="relu", colstat=torch.zeros(ops.colstat_floats(250, 256), device=dev))


def test_pool_kernels_on_f16_activations(dev):
    import ctypes as C
    from speech_diarization_amd import _native as N
    lib = N.load()
    g = torch.Generator().manual_seed(4)
    B, T, Cc = 3, 201, 512
    x = (torch.randn(B * T, Cc, generator=g) * 2 + 0.5).half()
    xd = x.to(dev)
    st = torch.empty(B, 2 * Cc, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(lib.sd_seg_mean_std_dt(xd.data_ptr(), N.SD_DT_F16, Cc, 0, B, T, Cc, 1, C.c_float(1e-12), st.data_ptr(), stream), "mean_std")
    xr = x.double().view(B, T, Cc)
    assert (st[:, :Cc].cpu().double() - xr.mean(1)).abs().max() < 1e-5
    assert (st[:, Cc:].cpu().double() - xr.std(1, unbiased=False)).abs().max() < 1e-5
    logit = (torch.randn(B * T, Cc, generator=g) * 3).half()
    out = torch.empty(B, 2 * Cc, device=dev)
    logit_d = logit.to(dev)
    N.check(lib.sd_asp_pool_dt(logit_d.data_ptr(), Cc, xd.data_ptr(), N.SD_DT_F16, Cc, B, T, Cc, C.c_float(1e-12), out.data_ptr(), stream), "asp")
    a = torch.softmax(logit.double().view(B, T, Cc), dim=1)
    mu = (a * xr).sum(1)
    assert (out[:, :Cc].cpu().double() - mu).abs().max() < 1e-5
    gate = torch.rand(B, Cc, generator=g)
    res = torch.randn(B * T, Cc, generator=g).half()
    y = torch.empty(B * T, Cc, device=dev, dtype=torch.float16)
    gate_d, res_d = gate.to(dev), res.to(dev)      # keep the device copies alive across the async launch
    N.check(lib.sd_se_scale_residual_dt(xd.data_ptr(), Cc, gate_d.data_ptr(), res_d.data_ptr(), Cc, 0, y.data_ptr(), Cc, 0,
                                        B, T, Cc, N.SD_DT_F16, stream), "se")
    ref = x.double() * gate.double().repeat_interleave(T, 0) + res.double()
    assert (y.cpu().double() - ref).abs().max() < 1e-2       # one f16 rounding of a value up to ~10


@pytest.mark.parametrize("width,B,n", [(128, 5, 16000), (128, 3, 32000)])
def test_ecapa_f16_small_geometry(dev, width, B, n):
    from oracle import pipeline_ref
    from speech_diarization_amd import synth
    from speech_diarization_amd.engine import EmbeddingEngine
    sd = synth.make_ecapa_state_dict(21, synth.EcapaConfig.small(width))
    wav = synth.synthetic_segments(3, B, n)
    got = EmbeddingEngine(sd, dev, precision="f16").embed(torch.from_numpy(wav).to(dev)).cpu().numpy()
    ref = pipeline_ref.encode_batch_ref(sd, wav, torch.float64)
    cd = _cos_dist(got, ref)
    assert cd.max() < 1e-4, cd                # north_star bar: 1e-3


@pytest.mark.parametrize("B,n", [(4, 32000), (2, 16000), (2, 8000), (1, 48000)])   # T = 201 / 101 / 51: fused attention pooling; 301: two-operator path
def test_ecapa_f16_full_geometry(dev, B, n):
    from oracle import pipeline_ref
    from speech_diarization_amd import synth
    from speech_diarization_amd.engine import EmbeddingEngine
    sd = synth.make_ecapa_state_dict(1234)
    wav = synth.synthetic_segments(0, B, n)
    eng = EmbeddingEngine(sd, dev, precision="f16")
    # the f16 forward: the features cast in front of the stem and, up to T = 212, the fused Res2Net chain behind its weight pack
    T = 1 + n // 160
    chain = ["chain_pack_kernel", f"res2net_chain_f16_kernel<{(T + 31) // 32}>"] if T <= 212 else []
    with expect_launches(exactly=chain, at_least=["cast_f32_f16_kernel"], family={"res2net_chain_f16_kernel", "chain_pack_kernel"}):
        got = eng.embed(torch.from_numpy(wav).to(dev)).cpu().numpy()
    ref = pipeline_ref.encode_batch_ref(sd, wav, torch.float64)
    cd = _cos_dist(got, ref)
    assert cd.max() < 1e-3, cd
    print("f16 full-geometry max cosine distance", cd.max())


def test_f16_and_f32_engines_give_the_same_clusters(dev):
    """identical cluster assignments from the f16 path, the f32 path and the CPU path"""
    from oracle import pipeline_ref
    from speech_diarization_amd import cluster, ops, synth
    from speech_diarization_amd.diarization_baseline import gather_windows, speech_windows
    from speech_diarization_amd.engine import EmbeddingEngine
    sd = synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(128))
    conv = synth.synthetic_conversation(40.0, 3, seed=2)
    speech = [(s, e) for s, e, _ in conv.turns]
    starts, _, _ = speech_windows(speech, len(conv.wav), 16000, 2.0, 0.25)
    wav = gather_windows(conv.wav, starts, 32000)
    labels = []
    for emb in (EmbeddingEngine(sd, dev, precision="f16").embed(torch.from_numpy(wav).to(dev)).cpu().numpy(),
                EmbeddingEngine(sd, dev, precision="f32").embed(torch.from_numpy(wav).to(dev)).cpu().numpy(),
                pipeline_ref.encode_batch_ref(sd, wav, torch.float32)):
        K = ops.cosine_affinity(torch.from_numpy(cluster.center(emb).astype(np.float32)).to(dev)).cpu().numpy()
        labels.append(cluster.relabel_by_first_appearance(cluster.spectral(K, 3)))
    assert np.array_equal(labels[0], labels[1]) and np.array_equal(labels[1], labels[2])
    assert len(set(labels[0].tolist())) == 3


# ---- fused Res2Net chain (sd_res2net_chain_f16): one kernel per SE-Res2Net block

def _chain_case(seed, B, T, dil, n=7, C=1024):
    g = torch.Generator().manual_seed(seed)
    r = (torch.randn(B * T, C, generator=g) * 0.7).half()
    layers = []
    for j in range(n):
        layers.append(dict(w=(torch.randn(128, 128, 3, generator=g) / np.sqrt(384)).half().float(), bias=torch.randn(128, generator=g) * 0.1,
                           scale=torch.rand(128, generator=g) + 0.5, shift=torch.randn(128, generator=g) * 0.1, dil=dil))
    return r, layers


def _chain_f64(r, layers, T):
    """float64 restatement with the path's own f16 roundings of the chain state (y_j and c_{j+1} + y_j)."""
    r = r.double().clone()
    n = len(layers)
    u = r[:, 128:256].clone()
    for j in range(1, n + 1):
        L = layers[j - 1]
        y = torch.relu(_ref_conv_cl(u, L["w"].double(), L["bias"].double(), T, L["dil"])) * L["scale"].double() + L["shift"].double()
        r[:, 128 * j:128 * j + 128] = y.half().double()
        if j < n:
            u = (y + r[:, 128 * (j + 1):128 * (j + 2)]).half().double()
    return r


@pytest.mark.parametrize("B,T,dil,n", [(5, 201, 2, 7), (3, 201, 3, 7), (4, 201, 4, 7), (6, 101, 2, 7), (2, 61, 3, 7), (3, 212, 4, 7),
                                       (2, 16, 2, 7), (1, 5, 4, 3), (2, 208, 2, 1),
                                       (2, 96, 2, 7), (2, 150, 3, 7), (2, 170, 2, 5), (2, 33, 2, 7), (1, 64, 3, 7), (1, 32, 2, 2)])   # every count of 32-row tiles, tile-aligned and one row over
def test_res2net_chain_matches_f64_and_the_unfused_convs(dev, B, T, dil, n):
    from speech_diarization_amd import ops
    assert ops.res2net_chain_supported(T, 128, n, 3, dil)
    r, layers = _chain_case(B * 1000 + T + dil, B, T, dil, n)
    ref = _chain_f64(r, layers, T)
    dl = [dict(w=ops.pack_weight(L["w"], dev, torch.float16), bias=L["bias"].to(dev), scale=L["scale"].to(dev), shift=L["shift"].to(dev), dil=dil)
          for L in layers]
    got = r.to(dev).clone()
    ops.res2net_chain(got, T, dl)
    torch.cuda.synchronize()
    got = got.cpu().double()
    assert torch.equal(got[:, :128], r[:, :128].double())                           # chunk 0 untouched
    if 128 * (n + 1) < r.shape[1]:
        assert torch.equal(got[:, 128 * (n + 1):], r[:, 128 * (n + 1):].double())   # chunks past the chain untouched
    scale = ref[:, 128:128 * (n + 1)].abs().max().item()
    err = (got - ref)[:, 128:128 * (n + 1)].abs().max().item()
    # one f16 ulp of a chain-state rounding can flip (the MFMA sums in another order than float64) and then propagates
    assert err < 4e-3 * scale, (err, scale)
    # the unfused path: the same operators launched one by one (tee epilogue), same roundings -> same values to f16 rounding flips
    un = r.to(dev).clone()
    s0 = un[:, 128:256].clone()
    s1 = torch.empty_like(s0)
    for j in range(1, n + 1):
        src, dst = (s0, s1) if j & 1 else (s1, s0)
        L = dl[j - 1]
        kw = dict(cin=128, dil=dil, bias=L["bias"], act="relu", scale=L["scale"], shift=L["shift"], out=un, o_col0=128 * j)
        if j < n:
            kw.update(tee=dst, tee_lo=0, tee_hi=128, tee_add=un, ta_col0=128 * (j + 1))
        ops.conv1d_cl(src, L["w"], T, **kw)
    torch.cuda.synchronize()
    d = (un.cpu().double() - got)[:, 128:128 * (n + 1)].abs()
    assert d.max().item() < 4e-3 * scale and (d > 0).double().mean().item() < 0.05, (d.max().item(), (d > 0).double().mean().item())


def test_res2net_chain_refuses_what_it_does_not_cover(dev):
    from speech_diarization_amd import _native, ops
    assert not ops.res2net_chain_supported(213, 128, 7, 3, 2)      # three [T][128] f16 buffers no longer fit the LDS
    assert not ops.res2net_chain_supported(201, 64, 7, 3, 2)
    assert not ops.res2net_chain_supported(201, 128, 8, 3, 2)
    assert not ops.res2net_chain_supported(201, 128, 7, 5, 2)
    assert not ops.res2net_chain_supported(3, 128, 7, 3, 4)        # reflect padding needs dilation < T
    r, layers = _chain_case(1, 2, 626, 2)
    dl = [dict(w=ops.pack_weight(L["w"], dev, torch.float16), bias=L["bias"].to(dev), scale=L["scale"].to(dev), shift=L["shift"].to(dev), dil=2)
          for L in layers]
    before = r.to(dev)
    work = before.clone()
    with pytest.raises(_native.SdError, match="needs 1..7 convs"):
        ops.res2net_chain(work, 626, dl)
    assert torch.equal(work, before)                               # nothing was launched


def test_ecapa_f16_fused_and_unfused_res2net_agree(dev, monkeypatch):
    """The engine result with the chain kernel against the float64 oracle is covered by the full-geometry tests; here: a
    6 s segment (T = 601) takes the per-conv path and 2 s segments the fused one, both within the f16 bar."""
    from oracle import pipeline_ref
    from speech_diarization_amd import synth
    from speech_diarization_amd.engine import EmbeddingEngine
    sd = synth.make_ecapa_state_dict(1234)
    eng = EmbeddingEngine(sd, dev, precision="f16")
    for n in (32000, 96000):
        wav = synth.synthetic_segments(3, 2, n)
        e = eng.embed(torch.from_numpy(wav).to(dev)).cpu().numpy()
        ref = pipeline_ref.encode_batch_ref(sd, wav, torch.float64)
        assert _cos_dist(e, ref).max() < 1e-5


def test_fused_f16_pooling_bounds_the_cancellation(dev):
    """asp_attend_pool_f16_kernel forms the weighted variance as E_w[h^2] - mu^2 (the oracle: sum a (h - mu)^2).  Known-answer
    case with |mu| >> sigma: h = 50 + 0.01 noise.  f32 accumulation of f16 products keeps the difference to ~50^2 * 2^-22 / sigma."""
    from speech_diarization_amd import ops
    g = torch.Generator().manual_seed(11)
    B, T, Cc, att = 3, 201, 512, 128
    a1 = torch.tanh(torch.randn(B * T, att, generator=g)).half()
    wc = (torch.randn(Cc, att, 1, generator=g) / 4).half()
    for mean, sigma in ((50.0, 0.01), (8.0, 0.05), (-20.0, 0.02)):
        h = (mean + sigma * torch.randn(B * T, Cc, generator=g)).half()          # f16 spacing at 50 is 0.03: few distinct values
        got = ops.asp_attend_pool(a1.to(dev), ops.pack_weight(wc.float(), dev, torch.float16), h.to(dev), B, T).cpu().double()
        a = torch.softmax((a1.double() @ wc[:, :, 0].double().T).view(B, T, Cc), dim=1)
        hr = h.double().view(B, T, Cc)
        mu = (a * hr).sum(1)
        sd = torch.sqrt(((a * (hr - mu[:, None]) ** 2).sum(1)).clamp_min(1e-12))
        assert (got[:, :Cc] - mu).abs().max() < 2e-5 * max(1.0, abs(mean))
        # absolute error of the variance ~ mean^2 * 2^-21 -> of the std ~ that / (2 sd)
        bound = (mean * mean * 2.0 ** -21) / (2 * sd.min().item()) + 2e-4
        assert (got[:, Cc:] - sd).abs().max() < bound, (mean, sigma, (got[:, Cc:] - sd).abs().max().item(), bound)
        assert torch.isfinite(got).all() and (got[:, Cc:] >= 0).all()


def test_identical_clusters_at_full_geometry(dev):
    """north_star: 'identical cluster assignments on the same inputs' — f16 path, f32 path and the CPU oracle at the
    full C = 1024 geometry (the width-128 twin of this test runs more windows)."""
    from oracle import pipeline_ref
    from speech_diarization_amd import cluster, ops, synth
    from speech_diarization_amd.diarization_baseline import gather_windows, speech_windows
    from speech_diarization_amd.engine import EmbeddingEngine
    sd = synth.make_ecapa_state_dict(1234)
    conv = synth.synthetic_conversation(30.0, 3, seed=2)
    speech = [(s, e) for s, e, _ in conv.turns]
    starts, _, _ = speech_windows(speech, len(conv.wav), 16000, 2.0, 0.5)
    wav = gather_windows(conv.wav, starts, 32000)
    embs = [EmbeddingEngine(sd, dev, precision="f16").embed(torch.from_numpy(wav).to(dev)).cpu().numpy(),
            EmbeddingEngine(sd, dev, precision="f32").embed(torch.from_numpy(wav).to(dev)).cpu().numpy(),
            pipeline_ref.encode_batch_ref(sd, wav, torch.float32)]
    labels = []
    for emb in embs:
        K = ops.cosine_affinity(torch.from_numpy(cluster.center(emb).astype(np.float32)).to(dev)).cpu().numpy()
        labels.append((cluster.relabel_by_first_appearance(cluster.spectral(K, 3)),
                       cluster.relabel_by_first_appearance(cluster.ahc_cosine(K, 0.3))))
    for lab in labels[1:]:
        assert np.array_equal(lab[0], labels[0][0]) and np.array_equal(lab[1], labels[0][1])
    assert len(set(labels[0][0].tolist())) == 3
    assert _cos_dist(embs[0], embs[2]).max() < 1e-3 and _cos_dist(embs[1], embs[2]).max() < 1e-5


@pytest.mark.parametrize("mode", ["f16", "split16"])
def test_t256_lockstep_walk_gives_the_bits_of_the_hardware_dispatch(dev, mode):
    """Round 5: the 256x256 ring kernel's persistent lock-step walk (one workgroup per CU, XCD-contiguous static schedule;
    sd_set_tuning(SD_TUNE_T256_LOCKSTEP_TILES)) computes every tile exactly as the one-workgroup-per-tile launch does: bitwise equal outputs,
    also with a ragged last row tile, a tile count that is no multiple of 8, fewer tiles than CUs and several passes per workgroup."""
    from speech_diarization_amd import _native, ops
    lib = _native.load()
    g = torch.Generator().manual_seed(3)
    T = 201
    try:
        for B, cin, cout in ((3, 1024, 1024), (37, 1024, 1024), (350, 1024, 1024), (130, 3072, 3072)):
            M = B * T
            bias, scale, shift = torch.randn(cout, generator=g).to(dev), (torch.rand(cout, generator=g) + 0.5).to(dev), torch.randn(cout, generator=g).to(dev)
            w = torch.randn(cout, cin, 1, generator=g) / cin ** 0.5
            outs = []
            for thr in (1 << 40, 0):
                _native.check(lib.sd_set_tuning(_native.SD_TUNE_T256_LOCKSTEP_TILES, thr), "sd_set_tuning")
                if mode == "f16":
                    x = (torch.randn(M, cin, generator=g) * 0.5).half().to(dev) if not outs else x
                    wp = ops.pack_weight(w, dev, torch.float16)
                    y = torch.empty(M, cout, device=dev, dtype=torch.float16)
                    ops.conv1d_cl(x, wp, T, cin=cin, bias=bias, act="relu", scale=scale, shift=shift, out=y)
                else:
                    x = torch.randn(M, cin, generator=g).to(dev) if not outs else x
                    ws, s = ops.pack_weight_split16(w, dev)
                    y = ops.conv1d_cl_split16(x, ws, s, T, cin=cin, bias=bias, act="relu", scale=scale, shift=shift)
                outs.append(y)
            assert torch.equal(outs[0], outs[1]), (mode, B, cin, cout)
            assert bool(torch.isfinite(outs[1].float()).all())
    finally:
        _native.check(lib.sd_set_tuning(_native.SD_TUNE_T256_LOCKSTEP_TILES, -1), "sd_set_tuning")
