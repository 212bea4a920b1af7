"""Packed spans on the MI355X: segments of different lengths in one launch, each embedded as if it were alone.

The packed fbank is bitwise `sd_fbank_f32` of each span alone on both fbank routes; the packed conv and reductions match float64 per span
under every kernel selection of `sd_set_tuning`; `encode_spans` matches the float64 oracle of each span alone, the B = 1 call and, for equal
lengths, the uniform forward; permutations, NaN samples and duplicates stay in their rows bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
from launch_log import F32_CONV, expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu

BAR = {"f32": 1e-5}
FBANK_LENGTHS = [640, 799, 800, 9600, 32000, 32100, 32160, 100000, 480000]


def _cos_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


@pytest.fixture(params=["auto", "split32", "tiles128", "tiles64", "rows80", "rows96", "rows112", "wide256"])
def conv_kernel(request):
    """The eight kernel selections of the uniform operator (a copy of tests/test_gpu_short_segments.py's fixture): the packed layers must
    not care; the position-free layers of the packed forward take whichever the selection forces.  Tuning restored afterwards."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    N.check(lib.sd_set_tuning(N.SD_TUNE_S64_TILES, 0 if request.param != "auto" else -1), "sd_set_tuning")
    N.check(lib.sd_set_tuning(N.SD_TUNE_SKINNY_TILES, 0 if request.param not in ("auto", "split32") else -1), "sd_set_tuning")
    N.check(lib.sd_set_tuning(N.SD_TUNE_WIDE_TILES, 0 if request.param == "wide256" else -1), "sd_set_tuning")
    N.check(lib.sd_set_tuning(N.SD_TUNE_HALF_TILES, {"auto": -1, "split32": -1, "tiles64": 1}.get(request.param, 0)), "sd_set_tuning")
    N.check(lib.sd_set_tuning(N.SD_TUNE_TILE_ROWS, int(request.param[4:]) if request.param.startswith("rows") else (-1 if request.param in ("auto", "split32") else 0)), "sd_set_tuning")
    yield request.param
    N.check(lib.sd_set_tuning(N.SD_TUNE_HALF_TILES, -1), "sd_set_tuning")
    N.check(lib.sd_set_tuning(N.SD_TUNE_TILE_ROWS, -1), "sd_set_tuning")
    N.check(lib.sd_set_tuning(N.SD_TUNE_S64_TILES, -1), "sd_set_tuning")
    N.check(lib.sd_set_tuning(N.SD_TUNE_SKINNY_TILES, -1), "sd_set_tuning")
    N.check(lib.sd_set_tuning(N.SD_TUNE_WIDE_TILES, -1), "sd_set_tuning")


# ------------------------------------------------------------------ 1. fbank: bitwise the span alone, both routes

def test_fbank_packed_is_bitwise_the_span_alone(dev):
    from speech_diarization_amd import synth
    from speech_diarization_amd.engine import fbank_device, fbank_packed_device, span_frame_offsets
    from speech_diarization_amd.features import FbankPlan
    plan = FbankPlan("speechbrain", n_mels=80)
    total = 700000
    sig = torch.from_numpy(synth.synthetic_segments(11, 1, total)[0]).to(dev)
    g = np.random.default_rng(0)
    lengths = FBANK_LENGTHS + [640, 480000, 32100, 9600]
    starts = [int(g.integers(0, total - n)) for n in FBANK_LENGTHS]
    starts += [0, total - 480000, starts[5] + 17, starts[3] + 4000]        # both ends of the signal; overlapping spans
    order = g.permutation(len(lengths))                                    # the routes interleaved in the pack
    starts, lengths = [starts[i] for i in order], [lengths[i] for i in order]
    # both routes of the pack: the spans of up to 201 frames on the one-launch kernel, the longer ones tiled for the folded-DFT kernel
    with expect_launches(exactly=["fbank_utt16_kernel<packed>", "fbank_packed_tiles_kernel", "fill_i32_kernel", "fbank_logmel_kernel<packed>",
                                  "fbank_finalize_kernel<packed>"]):
        got = fbank_packed_device(sig, starts, lengths, plan)
    fs = span_frame_offsets(lengths)
    for s, (a, n) in enumerate(zip(starts, lengths)):
        alone = fbank_device(sig[a:a + n].contiguous()[None], plan)[0]
        assert torch.equal(got[fs[s]:fs[s + 1]], alone), (s, a, n)


# ------------------------------------------------------------------ 2. operators against float64, every kernel selection

def _spans_T(seed, lo, count, hi=3001):
    g = np.random.default_rng(seed)
    T = g.integers(lo, 60, count).tolist()
    T[0] = lo
    T[len(T) // 2] = hi
    return T


def _ref_conv(x, w, b, T_list, dil):
    out, r = [], 0
    pad = dil * (w.shape[2] - 1) // 2
    for T in T_list:
        xt = x[r:r + T].t()[None]
        if pad:
            xt = F.pad(xt, (pad, pad), mode="reflect")
        out.append(F.conv1d(xt, w, b, dilation=dil)[0].t())
        r += T
    return torch.cat(out)


def _offsets(T_list):
    return np.concatenate([[0], np.cumsum(T_list)]).astype(np.int32)


@pytest.mark.parametrize("k,dil,cin,cout", [(5, 1, 80, 1024), (3, 2, 128, 128), (3, 3, 128, 128), (3, 4, 128, 128)])
def test_packed_conv_matches_f64(dev, conv_kernel, k, dil, cin, cout):
    from speech_diarization_amd import ops
    T = _spans_T(k * 10 + dil, 1 + dil * (k - 1) // 2, 23)
    M = sum(T)
    g = torch.Generator().manual_seed(M + dil)
    x = torch.randn(M, cin, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, k, generator=g, dtype=torch.float64) / np.sqrt(cin * k)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    scale = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5
    shift = torch.randn(cout, generator=g, dtype=torch.float64)
    ref = torch.relu(_ref_conv(x, w, b, T, dil)) * scale + shift
    with expect_launches(exactly=["conv_gemm_f32_packed_kernel"], family=F32_CONV):      # whatever the selection: no other kernel has the span map
        got = ops.conv1d_cl_packed(x.float().to(dev), ops.pack_weight(w.float(), dev), _offsets(T), cin=cin, dil=dil, bias=b.float().to(dev),
                                   act="relu", scale=scale.float().to(dev), shift=shift.float().to(dev))
        torch.cuda.synchronize()
    err = (got.cpu().double() - ref).abs().max().item()
    assert err < 2e-5 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("T", [[5], [5, 7, 5, 9], None])
def test_packed_conv_epilogues_and_tile_counts(dev, conv_kernel, T):
    """per-segment bias + tee / tee_add + act2, from ONE 5-frame span (M = 5) up to a launch of over 1000 128x128 tiles"""
    from speech_diarization_amd import ops
    cin, cout, dil = 128, 128, 4
    if T is None:
        T = _spans_T(7, 5, 400, 3001) * 3                                 # ~ 150 k rows x 128: > 1000 tiles
    M = sum(T)
    g = torch.Generator().manual_seed(len(T))
    x = torch.randn(M, cin + 64, generator=g, dtype=torch.float64)
    w = torch.randn(cout, cin, 3, generator=g, dtype=torch.float64) / np.sqrt(3 * cin)
    segb = torch.randn(len(T), cout, generator=g, dtype=torch.float64)
    add = torch.randn(M, cout, generator=g, dtype=torch.float64)
    tee = torch.zeros(M, cout, device=dev)
    got = ops.conv1d_cl_packed(x.float().to(dev), ops.pack_weight(w.float(), dev), _offsets(T), cin=cin, dil=dil, bias=segb.float().to(dev),
                               bias_per_seg=True, act="relu", act2="sigmoid", a_col0=64, tee=tee, tee_lo=0, tee_hi=cout,
                               tee_add=add.float().to(dev), ta_col0=0)
    torch.cuda.synchronize()
    y = _ref_conv(x[:, 64:].contiguous(), w, None, T, dil) + segb.repeat_interleave(torch.tensor(T), dim=0)
    y = torch.sigmoid(torch.relu(y))
    assert (got.cpu().double() - y).abs().max() < 1e-5
    assert (tee.cpu().double() - (y + add)).abs().max() < 1e-5


def test_packed_reductions_match_f64(dev, conv_kernel):
    from speech_diarization_amd import ops
    T = _spans_T(5, 5, 17)
    fs = _offsets(T)
    M, Cc = sum(T), 512
    g = torch.Generator().manual_seed(9)
    x = torch.randn(M, Cc, generator=g, dtype=torch.float64)
    lg = torch.randn(M, Cc, generator=g, dtype=torch.float64)
    gate = torch.rand(len(T), Cc, generator=g, dtype=torch.float64)
    res = torch.randn(M, Cc, generator=g, dtype=torch.float64)
    xd = x.float().to(dev)
    with expect_launches(exactly=["seg_mean_std_kernel<f32,packed,64x4>", "asp_pool_kernel<f32,packed>", "se_scale_residual_kernel<f32,packed>"],
                         family={"seg_mean_std_kernel", "asp_pool_kernel", "asp_pool_lds_kernel", "se_scale_residual_kernel"}):
        st = ops.seg_mean_std_packed(xd, fs).cpu().double()
        pool = ops.asp_pool_packed(lg.float().to(dev), xd, fs).cpu().double()
        y = ops.se_scale_residual_packed(xd, gate.float().to(dev), res.float().to(dev), fs).cpu().double()
    for s in range(len(T)):
        xs, ls = x[fs[s]:fs[s + 1]], lg[fs[s]:fs[s + 1]]
        mu = xs.mean(0)
        assert (st[s, :Cc] - mu).abs().max() < 1e-5 and (st[s, Cc:] - xs.std(0, unbiased=False)).abs().max() < 1e-5
        a = torch.softmax(ls, 0)
        pm = (a * xs).sum(0)
        psd = torch.sqrt(((a * (xs - pm) ** 2).sum(0)).clamp_min(1e-12))
        assert (pool[s, :Cc] - pm).abs().max() < 1e-5 and (pool[s, Cc:] - psd).abs().max() < 1e-5
        assert (y[fs[s]:fs[s + 1]] - (xs * gate[s] + res[fs[s]:fs[s + 1]])).abs().max() < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_equal_spans_are_bitwise_the_uniform_reductions(dev, dtype):
    """One kernel per operator, two segment maps: spans of one length, in a pack big enough for the uniform operators' 64 x 4 shape
    (C = 1024, B = 64: grid.x * B = 256) and, at T = 300, their streaming pooling kernel (a segment's tile above the LDS kernel's 64 KB),
    give bitwise the uniform operator's result."""
    from speech_diarization_amd import _native as N, ops
    lib = N.load()
    B, Cc, dt = 64, 1024, ops._dt(dtype)
    g = torch.Generator().manual_seed(21)
    for T in (37, 300):
        M = B * T
        fs = np.arange(B + 1, dtype=np.int32) * T
        x = torch.randn(M, Cc, generator=g).to(dev, dtype)
        s = ops._stream(x)
        if T == 37:
            st = torch.empty(B, 2 * Cc, device=dev)
            N.check(lib.sd_seg_mean_std_dt(x.data_ptr(), dt, Cc, 0, B, T, Cc, 1, C.c_float(1e-12), st.data_ptr(), s), "sd_seg_mean_std_dt")
            assert torch.equal(ops.seg_mean_std_packed(x, fs), st)
            gate = torch.rand(B, Cc, generator=g).to(dev)
            res = torch.randn(M, Cc, generator=g).to(dev, dtype)
            y = torch.empty_like(x)
            N.check(lib.sd_se_scale_residual_dt(x.data_ptr(), Cc, gate.data_ptr(), res.data_ptr(), Cc, 0, y.data_ptr(), Cc, 0, B, T, Cc, dt, s),
                    "sd_se_scale_residual_dt")
            assert torch.equal(ops.se_scale_residual_packed(x, gate, res, fs), y)
        else:
            lg = torch.randn(M, Cc, generator=g).to(dev, dtype)
            pool = torch.empty(B, 2 * Cc, device=dev)
            N.check(lib.sd_asp_pool_dt(lg.data_ptr(), Cc, x.data_ptr(), dt, Cc, B, T, Cc, C.c_float(1e-12), pool.data_ptr(), s), "sd_asp_pool_dt")
            assert torch.equal(ops.asp_pool_packed(lg, x, fs), pool)


# ------------------------------------------------------------------ 3 - 8. the whole path

_CACHE = {}


def _state(name="full"):
    from speech_diarization_amd import synth
    if name not in _CACHE:
        cfg = synth.EcapaConfig(channels=(512, 512, 512, 512, 1536)) if name == "c512" else None
        _CACHE[name] = synth.make_ecapa_state_dict(1234, cfg) if cfg is not None else synth.make_ecapa_state_dict(1234)
    return _CACHE[name]


def _encoder(dev, name="full", max_batch=512):
    from speech_diarization_amd.speech_encode import HipEcapaEncoder
    key = ("enc", name, max_batch)
    if key not in _CACHE:
        _CACHE[key] = HipEcapaEncoder(_state(name), dev, max_batch=max_batch)
    return _CACHE[key]


def _pack(secs, seed=100):
    """one signal holding the spans back to back with gaps; the 0.3 .. 30 s lengths of test_gpu_wav_lens._ragged_batch + 640 samples"""
    from speech_diarization_amd import synth
    lens = [int(s * 16000) for s in secs]
    pieces, starts, at = [], [], 0
    for i, n in enumerate(lens):
        gap = synth.synthetic_segments(seed + 50 + i, 1, 1234)[0]
        pieces += [gap, synth.synthetic_segments(seed + i, 1, n)[0]]
        starts.append(at + gap.size)
        at += gap.size + n
    return np.concatenate(pieces).astype(np.float32), np.array(starts, np.int64), np.array(lens, np.int64)


RAGGED = [0.3, 1.0, 2.5, 4.0, 7.5, 12.0, 20.0, 30.0, 0.04]


def _ref(name, sig, starts, lens):
    from oracle import pipeline_ref
    key = ("ref", name, sig.size, tuple(starts.tolist()), tuple(lens.tolist()))
    if key not in _CACHE:
        _CACHE[key] = np.concatenate([pipeline_ref.encode_batch_ref(_state(name), sig[None, a:a + n]) for a, n in zip(starts, lens)])
    return _CACHE[key]


def test_encode_spans_full_geometry(dev):
    enc = _encoder(dev)
    sig, starts, lens = _pack(RAGGED)
    got = enc.encode_spans(sig, starts, lens)
    cd = _cos_dist(got, _ref("full", sig, starts, lens))
    print(f"\nencode_spans vs float64, per span: max cosine distance {cd.max():.2e}")
    assert np.isfinite(got).all() and cd.max() < BAR["f32"], cd
    alone = np.concatenate([enc.encode_batch(torch.from_numpy(sig[a:a + n].copy())[None]).squeeze(1).cpu().numpy() for a, n in zip(starts, lens)])
    assert _cos_dist(got, alone).max() < 1e-6
    # equal lengths: the uniform forward on the [B][n] matrix
    n = 32000
    eq_starts = np.array([0, 40000, 90000, 150000], np.int64)
    mat = np.stack([sig[a:a + n] for a in eq_starts])
    uni = enc.encode_batch(torch.from_numpy(mat)).squeeze(1).cpu().numpy()
    assert _cos_dist(enc.encode_spans(sig, eq_starts, np.full(4, n)), uni).max() < 1e-6


def test_encode_spans_every_kernel_selection(dev, conv_kernel):
    enc = _encoder(dev)
    sig, starts, lens = _pack([0.3, 1.0, 2.5, 0.04, 4.0], seed=300)
    cd = _cos_dist(enc.encode_spans(sig, starts, lens), _ref("full", sig, starts, lens))
    assert cd.max() < BAR["f32"], (conv_kernel, cd)


def test_encode_spans_c512_geometry(dev):
    enc = _encoder(dev, "c512")
    sig, starts, lens = _pack([30.0, 0.3, 2.0, 0.04, 7.5], seed=400)
    cd = _cos_dist(enc.encode_spans(sig, starts, lens), _ref("c512", sig, starts, lens))
    print(f"\nC = 512 geometry: max cosine distance {cd.max():.2e}")
    assert cd.max() < BAR["f32"], cd


def test_invariances_bit_for_bit(dev):
    enc = _encoder(dev)
    sig, starts, lens = _pack([0.3, 1.0, 2.5, 4.0, 7.5, 12.0, 0.04, 3.3], seed=500)
    base = enc.encode_spans(sig, starts, lens)
    perm = np.random.default_rng(1).permutation(len(lens))
    assert np.array_equal(enc.encode_spans(sig, starts[perm], lens[perm]), base[perm])
    bad = sig.copy()
    bad[starts[3] + 100] = np.nan
    got = enc.encode_spans(bad, starts, lens)
    assert np.isnan(got[3]).all()
    keep = [i for i in range(len(lens)) if i != 3]
    assert np.array_equal(got[keep], base[keep])
    dup = enc.encode_spans(sig, np.concatenate([starts, starts[[2, 2, 5]]]), np.concatenate([lens, lens[[2, 2, 5]]]))
    assert np.array_equal(dup[len(lens):], base[[2, 2, 5]]) and np.array_equal(dup[len(lens)], dup[len(lens) + 1])
    split = enc.encode_spans(sig, starts, lens, frame_budget=300)          # several calls, an over-budget span alone
    assert _cos_dist(split, base).max() < 1e-6


def test_refusals_before_launch(dev):
    from speech_diarization_amd.speech_encode import HipEcapaEncoder
    enc = _encoder(dev)
    sig = np.zeros(20000, np.float32)
    for st, ln in (([0], [639]), ([19500], [640]), ([-1], [640]), ([0, 10], [640])):
        with pytest.raises(ValueError):
            enc.encode_spans(sig, st, ln)
    with pytest.raises(ValueError, match="640 samples"):
        enc.encode_spans(sig, [0], [639])
    f16 = HipEcapaEncoder(_state(), dev, precision="f16")
    with pytest.raises(NotImplementedError, match="f32"):
        f16.encode_spans(sig, [0], [640])
    assert enc.encode_spans(sig, [], []).shape == (0, 192)


def test_encode_list_and_pipeline_opt_in(dev, monkeypatch):
    from speech_diarization_amd import anti_stick_diarize as A
    from speech_diarization_amd import speech_encode
    from speech_diarization_amd.anti_stick_diarize import Segment
    enc = _encoder(dev)
    monkeypatch.setattr(speech_encode, "using_ecapa_encoder", lambda *a, **k: enc)
    sig, starts, lens = _pack([0.3, 1.0, 2.5, 4.0], seed=600)
    wavs = [sig[a:a + n] for a, n in zip(starts, lens)]
    lst = speech_encode.ecapa_encode_list(wavs)
    assert lst.shape == (4, 192) and np.array_equal(lst, enc.encode_spans(sig, starts, lens))
    sr = 16000
    segs = [Segment(0.1, 0.35), Segment(0.5, 2.0), Segment(2.0, 2.2), Segment(3.0, 9.5), Segment(9.6, 11.9)]
    from speech_diarization_amd import synth
    y = synth.synthetic_segments(601, 1, 12 * sr)[0]
    got = A.embed_segments(y, sr, segs, packed=True)
    single = []
    for seg in segs:
        s, e = int(seg.start * sr), int(seg.end * sr)
        piece = y[s:e] if e - s >= 8000 else y[max(0, s - 2400): min(len(y), e + 2400)]
        single.append(enc.encode_batch(torch.from_numpy(piece.copy())[None]).squeeze(1).cpu().numpy())
    assert _cos_dist(got, np.concatenate(single)).max() < 1e-6
    assert np.array_equal(A.embed_segments(y, sr, segs, packed=False), A.embed_segments(y, sr, segs))


def test_meeting_sized_pack(dev):
    from speech_diarization_amd import synth
    enc = _encoder(dev)
    g = np.random.default_rng(7)
    secs = np.exp(g.uniform(np.log(0.3), np.log(20.0), 2000))
    lens = (secs * 16000).astype(np.int64)
    total = int(lens.sum() // 3 + 480000)
    sig = synth.synthetic_segments(77, 1, total)[0]
    starts = np.array([int(g.integers(0, total - n)) for n in lens], np.int64)
    got = enc.encode_spans(sig, starts, lens)
    assert got.shape == (2000, 192) and np.isfinite(got).all()
    for i in g.choice(2000, 16, replace=False):
        alone = enc.encode_batch(torch.from_numpy(sig[starts[i]:starts[i] + lens[i]].copy())[None]).squeeze(1).cpu().numpy()
        assert _cos_dist(got[i:i + 1], alone).max() < 1e-6, i
