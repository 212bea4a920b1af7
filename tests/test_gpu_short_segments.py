"""Parity along the segment-length axis, from the shortest segment the network takes (T = 5 frames, 640 samples) up past every
point where the ECAPA schedule (sd_ecapa.hip) changes route as T grows.

At short T one 64 .. 256-row tile spans tens of segments and the reflect padding of the dilation-4 Res2Net convs reaches the far end of
every segment: each operator is compared here with a float64 torch reference that pads with `F.pad(mode="reflect")` (so the reference
itself refuses what speechbrain refuses), then the whole forward with `pipeline_ref.encode_batch_ref(..., float64)` at every precision."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from kernel_selection import PINNED_LABEL, conv_kernel, f16_tiles, f32_conv_label  # noqa: E402,F401  (the selections of the f32 and the f16 / split16 convs, shared fixtures)
from launch_log import F32_CONV, expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu

PRECISIONS = ["f32", "f32ns", "f32s", "f16"]
BAR = {"f32": 1e-5, "f32ns": 1e-5, "f32s": 1e-5, "f16": 1e-3}
TILE_ROWS = (32, 64, 80, 96, 112, 128, 256)


def _cos_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def _ref_conv_cl(x, w, b, T, dil):
    """x [M, cin] channel-last, w [cout, cin, k]; 'same' reflect conv per segment (F.pad raises for pad >= T)."""
    M, cin = x.shape
    xt = x.view(M // T, T, cin).transpose(1, 2)
    pad = dil * (w.shape[2] - 1) // 2
    if pad:
        xt = F.pad(xt, (pad, pad), mode="reflect")
    return F.conv1d(xt, w, b, dilation=dil).transpose(1, 2).reshape(M, -1)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# (B, T, cin, cout, k, dil): T = pad + 1 for every (k, dil) of the network, then a few frames more; M = B * T is a multiple of no
# tile height, so every kernel sees a partial last tile with tens of segments in each full one
SHORT_SHAPES = [
    (53, 3, 80, 1024, 5, 1),        # stem at its floor (pad 2): 85 segments per 256-row tile
    (97, 3, 128, 128, 3, 2),        # Res2Net, block 1 (pad 2)
    (71, 4, 128, 128, 3, 3),        # Res2Net, block 2 (pad 3)
    (59, 5, 128, 128, 3, 4),        # Res2Net, block 3 (pad 4): the network's floor
    (45, 6, 128, 128, 3, 4),
    (37, 7, 1024, 3072, 1, 1),      # MFA-wide output
    (29, 9, 80, 1024, 5, 1),
    (23, 16, 128, 128, 3, 4),
    (19, 17, 1024, 1024, 1, 1),     # tdnn1 / tdnn2
    (33, 7, 3072, 128, 1, 1),       # attention TDNN: K = 3072
]


def test_short_shapes_are_a_multiple_of_no_tile_height():
    for B, T, *_ in SHORT_SHAPES:
        assert all((B * T) % h for h in TILE_ROWS), (B, T)


def _conv_case(seed, B, T, cin, cout, k):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * T, cin, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, k, generator=g, dtype=torch.float64) / np.sqrt(cin * k)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    scale = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5
    shift = torch.randn(cout, generator=g, dtype=torch.float64)
    return x, w, b, scale, shift


# ------------------------------------------------------------------ 1. the exact-f32 conv, all eight kernel selections

@pytest.mark.parametrize("B,T,cin,cout,k,dil", SHORT_SHAPES)
def test_short_conv1d_cl_f32_matches_f64(dev, conv_kernel, B, T, cin, cout, k, dil):
    from speech_diarization_amd import ops
    x, w, b, scale, shift = _conv_case(B * 1000 + T + cout, B, T, cin, cout, k)
    ref = torch.relu(_ref_conv_cl(x, w, b, T, dil)) * scale + shift
    with expect_launches(exactly=[f32_conv_label(conv_kernel, B * T, T, cout)], family=F32_CONV):
        got = ops.conv1d_cl(x.float().to(dev), ops.pack_weight(w.float(), dev), T, cin=cin, dil=dil, bias=b.float().to(dev),
                            act="relu", scale=scale.float().to(dev), shift=shift.float().to(dev))
        torch.cuda.synchronize()
    err = (got.cpu().double() - ref).abs().max().item()
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("B,T,cin,cout,dil", [(61, 5, 128, 128, 4),      # Res2Net step: per-segment bias, sigmoid, tee + tee_add
                                              (77, 3, 128, 1024, 2),     # wide output (takes no tee_add): tee only
                                              (51, 7, 96, 1100, 3)])     # wide, cout % 8 != 0: the scalar epilogue
def test_short_conv1d_cl_f32_epilogues(dev, conv_kernel, B, T, cin, cout, dil):
    """The epilogue at short T: a per-segment bias changes every few rows inside one tile, act2 after the affine, tee (+ tee_add)."""
    from speech_diarization_amd import ops
    g = torch.Generator().manual_seed(B + T + cout)
    lda = cin + 64
    xbig = torch.randn(B * T, lda, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, generator=g, dtype=torch.float64) / np.sqrt(3 * cin)
    segb = torch.randn(B, cout, generator=g, dtype=torch.float64)
    scale = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5
    shift = torch.randn(cout, generator=g, dtype=torch.float64)
    add = torch.randn(B * T, cout, generator=g, dtype=torch.float64)
    xd, add_d = xbig.float().to(dev), add.float().to(dev)
    hid = min(cout, 128)
    tee = torch.zeros(B * T, hid, device=dev)
    with_add = cout <= 256
    kw = dict(cin=cin, dil=dil, bias=segb.float().to(dev), bias_per_seg=True, act="relu", scale=scale.float().to(dev),
              shift=shift.float().to(dev), act2="sigmoid", a_col0=64, tee=tee, tee_lo=0, tee_hi=hid)
    if with_add:
        kw.update(tee_add=add_d, ta_col0=0)
    with expect_launches(exactly=[f32_conv_label(conv_kernel, B * T, T, cout, tee_add=with_add)], family=F32_CONV):
        got = ops.conv1d_cl(xd, ops.pack_weight(w.float(), dev), T, **kw)
        torch.cuda.synchronize()
    y = _ref_conv_cl(xbig[:, 64:].contiguous(), w, None, T, dil) + segb.repeat_interleave(T, dim=0)
    y = torch.sigmoid(torch.relu(y) * scale + shift)
    assert (got.cpu().double() - y).abs().max() < 1e-5
    want_tee = y[:, :hid] + (add[:, :hid] if with_add else 0.0)
    assert (tee.cpu().double() - want_tee).abs().max() < 1e-5


# ------------------------------------------------------------------ 2. the f16 and split16 convs

@pytest.mark.parametrize("B,T,cin,cout,k,dil", SHORT_SHAPES)
def test_short_conv1d_cl_f16_matches_f64(dev, f16_tiles, B, T, cin, cout, k, dil):
    from speech_diarization_amd import ops
    x, w, b, scale, shift = _conv_case(B * 77 + T + cout, B, T, cin, cout, k)
    xdt = torch.float32 if cin == 80 else torch.float16             # the stem reads the f32 features
    ydt = torch.float32 if cout == 3072 else torch.float16
    xq, wq = x.to(xdt), w.half()
    # reference on the same rounded operands, float64 arithmetic: accumulation + output rounding only
    ref = torch.relu(_ref_conv_cl(xq.double(), wq.double(), b, T, dil)) * scale + shift
    got = ops.conv1d_cl(xq.to(dev), ops.pack_weight(w.float(), dev, torch.float16), T, cin=cin, dil=dil, bias=b.float().to(dev),
                        act="relu", scale=scale.float().to(dev), shift=shift.float().to(dev), out_dtype=ydt)
    torch.cuda.synchronize()
    assert got.dtype == ydt
    tol = (1e-3 if ydt == torch.float16 else 2e-5) * max(1.0, ref.abs().max().item())
    assert (got.cpu().double() - ref).abs().max().item() < tol


@pytest.mark.parametrize("B,T,cout", [(85, 3, 1024), (61, 5, 1100), (37, 7, 1032)])
def test_short_conv1d_cl_f16_staged_epilogue(dev, f16_tiles, B, T, cout):
    """The 256x256 kernel's LDS-staged epilogue (not the "plain" one): per-segment bias, act2, a tee and cout % 8 != 0."""
    from speech_diarization_amd import ops
    g = torch.Generator().manual_seed(B * T + cout)
    cin, chunk = 128, 128
    x = torch.randn(B * T, cin, generator=g).half()
    w = (torch.randn(cout, cin, 3, generator=g) / np.sqrt(3 * cin)).half()
    segb = torch.randn(B, cout, generator=g)
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    tee = torch.zeros(B * T, chunk, device=dev, dtype=torch.float16)
    out = ops.conv1d_cl(x.to(dev), ops.pack_weight(w.float(), dev, torch.float16), T, cin=cin, dil=2, bias=segb.to(dev), bias_per_seg=True,
                        act="relu", scale=scale.to(dev), shift=shift.to(dev), act2="sigmoid", tee=tee, tee_lo=chunk, tee_hi=2 * chunk,
                        out_dtype=torch.float16)
    torch.cuda.synchronize()
    ref = _ref_conv_cl(x.double(), w.double(), None, T, 2) + segb.double().repeat_interleave(T, dim=0)
    ref = torch.sigmoid(torch.relu(ref) * scale.double() + shift.double())
    assert (out.cpu().double() - ref).abs().max() < 1e-3
    assert torch.equal(tee, out[:, chunk:2 * chunk])


@pytest.mark.parametrize("B,T,cin,cout,k,dil", SHORT_SHAPES)
def test_short_conv1d_cl_split16_matches_f64(dev, f16_tiles, B, T, cin, cout, k, dil):
    """Narrow outputs (cout <= 256): the 128x128 kernel that splits f32 activations while staging them; wide ones: split16_pack + the
    256x256 kernel, with f32 and SD_DT_SPLIT16 outputs (the latter bit for bit the pack of the former)."""
    from speech_diarization_amd import ops
    x, w, b, scale, shift = _conv_case(B * 131 + T + cout, B, T, cin, cout, k)
    x[:, ::7] *= 1e-3                                                 # small and large channels side by side
    x, w = x.float().double(), w.float().double()                     # the f32 operands the kernel sees
    ref = torch.relu(_ref_conv_cl(x, w, b, T, dil)) * scale + shift
    ws, s = ops.pack_weight_split16(w.float(), dev)
    narrow = cout <= 256
    kw = dict(cin=cin, dil=dil, bias=b.float().to(dev), act="relu", scale=scale.float().to(dev), shift=shift.float().to(dev))
    xd = x.float().to(dev)
    got = ops.conv1d_cl_split16(xd, ws, s, T, narrow=narrow, **kw)
    torch.cuda.synchronize()
    top = ref.abs().max().item()
    assert (got.cpu().double() - ref).abs().max().item() < 2e-6 * max(1.0, top)
    if cout % 32 == 0:
        ysp = torch.zeros((B * T, 2 * cout), device=dev, dtype=torch.float16)
        ops.conv1d_cl_split16(xd, ws, s, T, narrow=narrow, out=torch.zeros_like(got), out_split=ysp, **kw)
        assert torch.equal(ysp, ops.split16_pack(got, 0, cout))


@pytest.mark.parametrize("B,T,cout", [(59, 5, 128), (85, 3, 256)])
def test_short_conv1d_cl_split16_narrow_epilogues(dev, f16_tiles, B, T, cout):
    """The narrow split kernel with what the Res2Net chain and the attention TDNN ask of it at short T: per-segment bias, act2, tee + tee_add."""
    from speech_diarization_amd import ops
    g = torch.Generator().manual_seed(B + T)
    cin = 128
    x = torch.randn(B * T, cin, generator=g).double()
    w = (torch.randn(cout, cin, 3, generator=g) / np.sqrt(3 * cin)).double()
    segb = torch.randn(B, cout, generator=g).double()
    scale = (torch.rand(cout, generator=g) + 0.5).double()
    shift = torch.randn(cout, generator=g).double()
    add = torch.randn(B * T, cout, generator=g).double()
    ws, s = ops.pack_weight_split16(w.float(), dev)
    tee = torch.zeros(B * T, cout, device=dev)
    got = ops.conv1d_cl_split16(x.float().to(dev), ws, s, T, narrow=True, cin=cin, dil=4 if T > 4 else 2, bias=segb.float().to(dev),
                                bias_per_seg=True, act="relu", scale=scale.float().to(dev), shift=shift.float().to(dev), act2="tanh",
                                tee=tee, tee_lo=0, tee_hi=cout, tee_add=add.float().to(dev), ta_col0=0)
    torch.cuda.synchronize()
    ref = _ref_conv_cl(x, w, None, T, 4 if T > 4 else 2) + segb.repeat_interleave(T, dim=0)
    ref = torch.tanh(torch.relu(ref) * scale + shift)
    assert (got.cpu().double() - ref).abs().max() < 2e-6
    assert (tee.cpu().double() - (ref + add)).abs().max() < 4e-6


@pytest.mark.parametrize("k,dil", [(5, 1), (3, 2), (3, 3), (3, 4)])
def test_short_conv_refuses_t_at_the_pad(dev, k, dil):
    """T = pad: a single reflection cannot reach; all three conv operators refuse it before launching, as F.pad does."""
    from speech_diarization_amd import _native, ops
    T = dil * (k - 1) // 2
    B, cin, cout = 7, 128, 128
    x = torch.randn(B * T, cin, dtype=torch.float64)
    w = torch.randn(cout, cin, k, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="Padding size"):
        _ref_conv_cl(x, w, None, T, dil)
    xd = x.float().to(dev)
    with pytest.raises(_native.SdError, match="reflect padding"):
        ops.conv1d_cl(xd, ops.pack_weight(w.float(), dev), T, cin=cin, dil=dil)
    with pytest.raises(_native.SdError, match="reflect padding"):
        ops.conv1d_cl(xd.half(), ops.pack_weight(w.float(), dev, torch.float16), T, cin=cin, dil=dil)
    ws, s = ops.pack_weight_split16(w.float(), dev)
    with pytest.raises(_native.SdError, match="reflect padding"):
        ops.conv1d_cl_split16(xd, ws, s, T, cin=cin, dil=dil, narrow=True)
    with pytest.raises(_native.SdError, match="reflect padding"):
        ops.conv1d_cl_split16(xd, ws, s, T, cin=cin, dil=dil)


# ------------------------------------------------------------------ 3. the fused Res2Net chain

def _chain_case(seed, B, T, dil, n=7, C_=1024):
    g = torch.Generator().manual_seed(seed)
    r = (torch.randn(B * T, C_, generator=g) * 0.7).half()
    layers = []
    for _ in range(n):
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


@pytest.mark.parametrize("B", [1, 7, 33])
@pytest.mark.parametrize("T,dil", [(T, d) for T in (5, 6, 7, 9, 13) for d in (2, 3, 4) if d < T])
def test_short_res2net_chain_matches_f64_and_the_unfused_convs(dev, B, T, dil):
    """The bars of test_gpu_f16.py: within 4e-3 of the largest output (about one f16 ulp) of float64 and of the unfused convs, and
    fewer than 5 % of the values differ from the unfused path -- that last one over at least 64 rows.  The two paths sum in different
    orders, so an f16 rounding of the chain state flips now and then, and the flip feeds every later step: over a handful of rows
    (B = 1, T = 5 .. 13: 5 .. 13 rows of 7 x 128 values) one early flip reaches a large share of the values.  Measured: 9.2 % at
    B = 1, T = 9, dil = 2 on the MI355X; two correct CPU chains, f32- and f64-accumulated with the same f16 state roundings, differ
    in 0 .. 9.1 % of the values at B = 1 (seeds 0 .. 4) and in 0.6 .. 3.5 % at 63 .. 402 rows."""
    from speech_diarization_amd import ops
    n = 7
    assert ops.res2net_chain_supported(T, 128, n, 3, dil)
    r, layers = _chain_case(B * 1000 + T * 10 + dil, B, T, dil, n)
    ref = _chain_f64(r, layers, T)
    dl = [dict(w=ops.pack_weight(L["w"], dev, torch.float16), bias=L["bias"].to(dev), scale=L["scale"].to(dev), shift=L["shift"].to(dev), dil=dil)
          for L in layers]
    got = r.to(dev).clone()
    ops.res2net_chain(got, T, dl)
    torch.cuda.synchronize()
    got = got.cpu().double()
    assert torch.equal(got[:, :128], r[:, :128].double())
    assert torch.equal(got[:, 128 * (n + 1):], r[:, 128 * (n + 1):].double())
    scale = ref[:, 128:128 * (n + 1)].abs().max().item()
    err = (got - ref)[:, 128:128 * (n + 1)].abs().max().item()
    assert err < 4e-3 * scale, (err, scale)                 # (the bar of test_gpu_f16.py: an f16 rounding flip of the chain state propagates)
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
    assert d.max().item() < 4e-3 * scale, d.max().item()
    if B * T >= 64:
        assert (d > 0).double().mean().item() < 0.05, (d > 0).double().mean().item()


def test_res2net_chain_length_limits():
    from speech_diarization_amd import ops
    assert ops.res2net_chain_supported(5, 128, 7, 3, 4) and not ops.res2net_chain_supported(4, 128, 7, 3, 4)
    assert ops.res2net_chain_supported(212, 128, 7, 3, 4) and not ops.res2net_chain_supported(213, 128, 7, 3, 4)


# ------------------------------------------------------------------ 4. pooling at short T, with and without relative lengths

def _pool_f64(logits, h, n_mask, eps=1e-12):
    B, T, Cc = h.shape
    mask = torch.arange(T)[None, :, None] < torch.as_tensor(n_mask)[:, None, None]
    a = torch.softmax(logits.masked_fill(~mask, float("-inf")), dim=1)
    mu = (a * h).sum(1)
    sd = torch.sqrt((a * (h - mu[:, None]) ** 2).sum(1).clamp_min(eps))
    return mu, sd


def _rel(T):
    """Relative lengths: all of it, one frame (n_mask = 1), about half, and a length that ends inside the last frame."""
    return torch.tensor([1.0, 0.9 / T, 0.5, (T - 0.5) / T], dtype=torch.float32)


SHORT_T = [2, 3, 5, 6, 7]


@pytest.mark.parametrize("mode", ["f32", "f16", "split16"])
@pytest.mark.parametrize("T", SHORT_T)
@pytest.mark.parametrize("lens", [False, True])
def test_short_fused_attention_pooling_matches_f64(dev, mode, T, lens):
    """f32 / split16: the bars of test_gpu_f16.py (2e-5).  f16: the kernel forms the variance as E_w[h^2] - mu^2 in f32, so the std
    carries an absolute error of about E_w[h^2] 2^-21 / (2 sd) on top of the 2e-4 bar (the model of
    test_fused_f16_pooling_bounds_the_cancellation); with two or three frames a channel's std is small far more often than with
    201 (sd = sqrt(a (1 - a)) |h_1 - h_0| at T = 2).  Measured: 6e-4 at T = 2 without lengths (a case whose smallest std is 2.2e-4)."""
    from speech_diarization_amd import _native as N
    from speech_diarization_amd import ops
    from speech_diarization_amd.features import length_frames
    lib = N.load()
    B, Cc, att = 4, 512, 128
    g = torch.Generator().manual_seed(T * 10 + lens)
    dtype = torch.float16 if mode == "f16" else torch.float32
    a1 = torch.tanh(torch.randn(B * T, att, generator=g)).to(dtype)
    wc = (torch.randn(Cc, att, 1, generator=g) / 4).to(dtype)
    h = (torch.randn(B * T, Cc, generator=g) * 1.5 + 0.3).to(dtype)
    rel = _rel(T)
    n_mask = length_frames(rel, T)[1] if lens else torch.full((B,), T)
    if lens:
        assert n_mask[1] == 1
    wp = ops.pack_weight(wc.float(), dev, dtype)
    dt = {"f32": N.SD_DT_F32, "f16": N.SD_DT_F16, "split16": N.SD_DT_SPLIT16}[mode]
    a1d, hd, rd = a1.to(dev), h.to(dev), rel.to(dev)
    got = torch.empty(B, 2 * Cc, device=dev)
    N.check(lib.sd_asp_attend_pool_lens_dt(a1d.data_ptr(), wp.data_ptr(), hd.data_ptr(), dt, Cc, B, T, rd.data_ptr() if lens else None, Cc, att,
                                           C.c_float(1e-12), got.data_ptr(), _stream()), "sd_asp_attend_pool_lens_dt")
    logits = (a1.double() @ wc[:, :, 0].double().T).view(B, T, Cc)
    mu, sd = _pool_f64(logits, h.double().view(B, T, Cc), n_mask)
    got = got.cpu().double()
    assert (got[:, :Cc] - mu).abs().max() < 2e-5
    if mode == "f16":
        e2 = (torch.softmax(logits.masked_fill(~(torch.arange(T)[None, :, None] < n_mask[:, None, None]), float("-inf")), dim=1)
              * h.double().view(B, T, Cc) ** 2).sum(1)
        sd_bar = e2 * 2.0 ** -21 / (2 * sd) + 2e-4
    else:
        sd_bar = torch.full_like(sd, 2e-5)
    live = n_mask > 1                 # one frame: sd = sqrt(clamp(0)) up to the f32 cancellation of the weighted variance
    assert bool(((got[live, Cc:] - sd[live]).abs() < sd_bar[live]).all()), ((got[:, Cc:] - sd).abs() / sd_bar)[live].max().item()
    if bool((~live).any()):
        assert got[~live, Cc:].abs().max() < 2e-3
    if not lens:
        assert torch.equal(got.float(), ops.asp_attend_pool(a1d, wp, hd, B, T, split16=mode == "split16").cpu())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("T", SHORT_T)
@pytest.mark.parametrize("lens", [False, True])
def test_short_asp_pool_and_seg_mean_std_match_f64(dev, dtype, T, lens):
    """The unfused pooling (`asp_pool`, after the logits conv) and the per-segment statistics (`seg_mean_std`: SE squeeze, global
    context) at short T."""
    from speech_diarization_amd import _native as N
    from speech_diarization_amd import ops
    from speech_diarization_amd.features import length_frames
    lib = N.load()
    B, Cc = 4, 768
    g = torch.Generator().manual_seed(T * 3 + lens)
    lg = (torch.randn(B * T, Cc, generator=g) * 2).to(dtype)
    h = (torch.randn(B * T, Cc, generator=g) * 1.5 + 0.3).to(dtype)
    rel = _rel(T)
    n_mask = length_frames(rel, T)[1] if lens else torch.full((B,), T)
    dt = N.SD_DT_F16 if dtype == torch.float16 else N.SD_DT_F32
    ld, hd, rd = lg.to(dev), h.to(dev), rel.to(dev)
    rp = rd.data_ptr() if lens else None
    got = torch.empty(B, 2 * Cc, device=dev)
    N.check(lib.sd_asp_pool_lens_dt(ld.data_ptr(), Cc, hd.data_ptr(), dt, Cc, B, T, rp, Cc, C.c_float(1e-12), got.data_ptr(), _stream()),
            "sd_asp_pool_lens_dt")
    mu, sd = _pool_f64(lg.double().view(B, T, Cc), h.double().view(B, T, Cc), n_mask)
    got = got.cpu().double()
    live = n_mask > 1
    assert (got[:, :Cc] - mu).abs().max() < 2e-5 and (got[live, Cc:] - sd[live]).abs().max() < 2e-5
    if not lens and dtype == torch.float32:           # the ops entry (sd_asp_pool_f32)
        plain = ops.asp_pool(ld, hd, B, T).cpu().double()
        assert (plain[:, :Cc] - mu).abs().max() < 2e-5 and (plain[:, Cc:] - sd).abs().max() < 2e-5
    st = torch.empty(B, 2 * Cc, device=dev)
    N.check(lib.sd_seg_mean_std_lens_dt(hd.data_ptr(), dt, Cc, 0, B, T, rp, Cc, 1, C.c_float(1e-12), st.data_ptr(), _stream()), "sd_seg_mean_std_lens_dt")
    hr = h.double().view(B, T, Cc)
    for b in range(B):
        xs = hr[b, : int(n_mask[b])]
        m = xs.mean(0)
        s = torch.sqrt(((xs - m) ** 2).mean(0).clamp_min(1e-12))
        assert (st[b, :Cc].cpu().double() - m).abs().max() < 2e-5
        if n_mask[b] > 1:
            assert (st[b, Cc:].cpu().double() - s).abs().max() < 2e-5
    if not lens and dtype == torch.float32:           # the ops entry (sd_seg_mean_std_f32)
        plain = ops.seg_mean_std(hd, B, T).cpu().double()
        assert (plain[:, :Cc] - hr.mean(1)).abs().max() < 2e-5
        assert (plain[:, Cc:] - hr.std(1, unbiased=False).clamp_min(1e-6)).abs().max() < 2e-5


# ------------------------------------------------------------------ 5. the forward along the length axis

# (T, extra samples past (T - 1) * 160): T = 1 + n // 160.  The routes a length takes (sd_ecapa.hip at the time of writing):
LENGTHS = [
    (5, 0), (5, 159),        # the floor: T = 1 + max pad; every Res2Net reflection reaches the far end of the segment
    (6, 0), (7, 0), (9, 0), (17, 0),
    (47, 0), (48, 0),        # 96-row f32 tiles take the epilogue's column statistics from T = 48
    (55, 0), (56, 159),      # 112-row tiles: from T = 56
    (63, 159), (64, 0),      # f32 / f16 column statistics from the epilogue at T >= 64; fused f32 pooling's 4-wave form up to 64
    (65, 0),                 # fused pooling: the next template above 64 frames
    (79, 0), (80, 0),        # 80-row tiles: colstat from T = 80
    (127, 0), (128, 159),    # split16 wide kernel: colstat from T = 128; fused pooling 8-tile form up to 128
    (129, 0),
    (192, 0), (193, 0),      # fused f16 pooling: 3-wave form up to 192
    (201, 0), (201, 62),     # 32 000 / 32 062 samples: utt16 fbank kernel; 32 100 is its last length (below)
    (208, 0), (209, 0),      # fused f32 pooling: 13-tile form up to 208
    (212, 0), (213, 0),      # fused f16 Res2Net chain up to T = 212 (three [T][128] f16 buffers in 160 KB of LDS), per-conv above
    (256, 0), (257, 159),    # fused attention + pooling up to T = 256; above it the logits conv + LDS-resident asp_pool
]
FBANK_SWITCH = [32100, 32102]    # the utt16 fbank kernel up to n = 32 100, the folded kernel from 32 102 (test_gpu_fbank_ecapa.py)

_SD = {}
_REF_CACHE = {}
_ENGINES = {}


def _sd():
    if "sd" not in _SD:
        from speech_diarization_amd import synth
        _SD["sd"] = synth.make_ecapa_state_dict(1234)
    return _SD["sd"]


def _case(n, B=3):
    """(wav [B, n], float64 oracle embeddings), computed once per length."""
    if (n, B) not in _REF_CACHE:
        from oracle import pipeline_ref
        from speech_diarization_amd import synth
        wav = synth.synthetic_segments(n + 7, B, n)
        wav[1] *= 0.05                                  # a quiet row
        _REF_CACHE[(n, B)] = (wav, pipeline_ref.encode_batch_ref(_sd(), wav, torch.float64))
    return _REF_CACHE[(n, B)]


def _engine(dev, precision, max_batch=512):
    from speech_diarization_amd.engine import EmbeddingEngine
    key = (precision, max_batch)
    if key not in _ENGINES:
        _ENGINES[key] = EmbeddingEngine(_sd(), dev, max_batch=max_batch, precision=precision)
    return _ENGINES[key]


def _check(got, ref, precision, what):
    cd = _cos_dist(got, ref)
    print(f"\n{what} {precision}: max cosine distance to float64 {cd.max():.2e}")
    assert np.isfinite(got).all() and cd.max() < BAR[precision], (what, cd)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [(T - 1) * 160 + extra for T, extra in LENGTHS] + FBANK_SWITCH)
def test_forward_along_the_length_axis_matches_f64(dev, precision, n):
    wav, ref = _case(n)
    got = _engine(dev, precision).embed(torch.from_numpy(wav).to(dev)).cpu().numpy()
    _check(got, ref, precision, f"n={n} T={1 + n // 160}")


@pytest.mark.parametrize("T", [5, 6, 9, 17])
def test_short_forward_under_every_f32_conv_selection(dev, conv_kernel, T):
    wav, ref = _case((T - 1) * 160)
    eng = _engine(dev, "f32")
    # (the full geometry has layers every pin applies to: time-axis convs for the row tiles, cout >= 1024 for the 256x256 kernel)
    with expect_launches(at_least=[PINNED_LABEL[conv_kernel]] if conv_kernel in PINNED_LABEL else []):
        got = eng.embed(torch.from_numpy(wav).to(dev)).cpu().numpy()
    _check(got, ref, "f32", f"T={T} {conv_kernel}")


def _sample_rows(B, T, k=64):
    """The first and last rows and rows whose segment straddles a tile edge of every height, spread over the launch."""
    rows = {0, B - 1}
    for h in TILE_ROWS:
        edges = [b for b in range(B) if (b * T) // h != (b * T + T - 1) // h]      # (none where T divides h)
        for q in (0, len(edges) // 3, 2 * len(edges) // 3, len(edges) - 1):
            if edges:
                rows.add(edges[q])
    rng = np.random.default_rng(B * T)
    while len(rows) < k:
        rows.add(int(rng.integers(0, B)))
    return sorted(rows)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B,n", [(4096, 640), (2048, 1600)])
def test_one_large_launch_of_short_segments(dev, precision, B, n):
    """One launch of thousands of 5- and 11-frame segments: the wide and 256-row kernels with ~50 segments per tile."""
    from oracle import pipeline_ref
    from speech_diarization_amd import synth
    T = 1 + n // 160
    wav = synth.synthetic_segments(B + n, B, n)
    rows = _sample_rows(B, T)
    assert len(rows) == 64 and rows[0] == 0 and rows[-1] == B - 1
    key = ("large", B, n)
    if key not in _REF_CACHE:
        _REF_CACHE[key] = pipeline_ref.encode_batch_ref(_sd(), wav[rows], torch.float64)
    got = _engine(dev, precision, max_batch=B).embed(torch.from_numpy(wav).to(dev))
    assert bool(torch.isfinite(got).all())
    _check(got[rows].cpu().numpy(), _REF_CACHE[key], precision, f"B={B} n={n}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_encode_batch_takes_the_640_sample_floor(dev, precision):
    """speechbrain embeds any n >= 640 (T >= 5 frames); n = 639 (T = 4) raises ValueError before anything is launched, on
    encode_batch and on embed_windows."""
    from speech_diarization_amd.speech_encode import HipEcapaEncoder
    wav, ref = _case(640)
    enc = HipEcapaEncoder(_sd(), dev, precision=precision)
    assert enc.engine.min_samples == 640
    got = enc.encode_batch(torch.from_numpy(wav)).squeeze(1).cpu().numpy()
    _check(got, ref, precision, "encode_batch n=640")
    fresh = enc.engine.sibling()                        # no workspace yet: a refusal must not allocate or launch
    with pytest.raises(ValueError, match="too short"):
        fresh.embed(torch.from_numpy(wav[:, :639]).to(dev))
    with pytest.raises(ValueError, match="too short"):
        fresh.embed_windows(torch.from_numpy(wav[0]).to(dev), torch.zeros(2, dtype=torch.int64), 639)
    assert fresh._ws is None
    with pytest.raises(ValueError, match="640 samples"):
        enc.encode_batch(torch.from_numpy(wav[:, :639]))
    # embed_windows at the floor: windows of one recording, bitwise embed() of the gathered rows, and the oracle
    sig = np.concatenate([wav[0], wav[1], wav[2]])
    starts = torch.tensor([0, 640, 1280], dtype=torch.int64)
    win = enc.engine.embed_windows(torch.from_numpy(sig).to(dev), starts, 640)
    assert torch.equal(win, enc.engine.embed(torch.from_numpy(wav).to(dev)))
    _check(win.cpu().numpy(), ref, precision, "embed_windows n=640")
