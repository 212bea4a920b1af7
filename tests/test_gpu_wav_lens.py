"""Relative lengths (speechbrain's wav_lens) on the MI355X: the device frame-count rule, the masked fbank mean on every fbank
route, each masked pooling operator against float64, and the full-geometry forward at every precision against the float64
speechbrain restatement in tests/helpers/wav_lens_ref.py.  The unmasked path must stay bit for bit what it was."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import wav_lens_ref as R  # noqa: E402
from launch_log import expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu

PRECISIONS = ["f32", "f32ns", "f32s", "f16"]
BAR = {"f32": 1e-5, "f32ns": 1e-5, "f32s": 1e-5, "f16": 1e-3}


def _cos_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from speech_diarization_amd import _native as N
    return N, N.load()


# ------------------------------------------------------------------ 1. the frame-count rule on the device

@pytest.mark.parametrize("T", [61, 201, 626, 3001])
def test_device_rule_equals_host_rule(dev, T):
    from speech_diarization_amd.features import length_frames
    N, lib = _lib()
    g = np.random.default_rng(T)
    edges = []
    for k in range(0, T + 1):
        for v in (k, k + 0.5):
            r = np.float32(v / T)
            edges += [r, np.nextafter(r, np.float32(0)), np.nextafter(r, np.float32(2))]
    rel = np.concatenate([g.uniform(0, 1, 1_000_000).astype(np.float32), np.array(edges, np.float32),
                          np.array([1e-30, 1e-7, 1.0], np.float32)])
    rel = np.clip(rel, np.float32(1e-30), np.float32(1.0))
    rd = torch.from_numpy(rel).to(dev)
    nn_ = torch.empty(rel.size, dtype=torch.int32, device=dev)
    nm_ = torch.empty_like(nn_)
    with expect_launches(exactly=["wav_lens_frames_kernel"]):
        N.check(lib.sd_wav_lens_frames(rd.data_ptr(), rel.size, T, nn_.data_ptr(), nm_.data_ptr(), _stream()), "sd_wav_lens_frames")
    hn, hm = length_frames(torch.from_numpy(rel), T)
    assert torch.equal(nn_.cpu().long(), hn) and torch.equal(nm_.cpu().long(), hm)
    N.check(lib.sd_wav_lens_frames(None, 5, T, nn_.data_ptr(), nm_.data_ptr(), _stream()), "sd_wav_lens_frames(NULL)")
    assert nn_[:5].tolist() == [T] * 5 and nm_[:5].tolist() == [T] * 5


# ------------------------------------------------------------------ 2. fbank: the masked sentence mean on all three routes

@pytest.mark.parametrize("route", ["utt16", "folded", "generic"])
def test_fbank_lens_matches_float64(dev, route):
    from speech_diarization_amd import synth
    from speech_diarization_amd.engine import fbank_device
    from speech_diarization_amd.features import FbankPlan
    N, lib = _lib()
    if route == "generic":
        plan, n, sr = FbankPlan("torchaudio", sr=8000), 40000, 8000
    else:
        plan, n, sr = FbankPlan("speechbrain"), (32000 if route == "utt16" else 100000), 16000
    B = 4
    wav = synth.synthetic_segments(n + 3, B, n)
    rel = np.array([1.0, 0.77, 0.5, 0.213], np.float32)
    for b in range(B):
        wav[b, int(rel[b] * n):] = 0.0                              # zero-padded tails, as the callers pad them
    wav[0, : n // 3] *= 0.01
    T = plan.frames(n)
    x = torch.from_numpy(wav).to(dev)
    rd = torch.from_numpy(rel).to(dev)
    out = torch.empty(B, T, 80, device=dev)
    ws = torch.empty(max(plan.workspace_bytes(B, n), 256), dtype=torch.uint8, device=dev)
    N.check(lib.sd_fbank_lens_f32(plan.handle, x.data_ptr(), B, n, rd.data_ptr(), out.data_ptr(), 80, ws.data_ptr(), ws.numel(), _stream()),
            "sd_fbank_lens_f32")
    got = out.cpu().numpy()
    if route == "generic":
        ref = R.torchaudio_fbank_lens_ref(wav, rel, sr=sr)
        tol = 2e-4
    else:
        ref = R.speechbrain_fbank_lens_ref(wav, rel)
        tol = 1e-3
    assert got.shape == ref.shape == (B, T, 80)
    assert np.abs(got - ref).max() < tol, np.abs(got - ref).max()
    # the per-row mean really moved: the unmasked features differ on the short rows
    plain = fbank_device(x, plan, mean_norm=True)
    assert np.abs(plain[3].cpu().numpy() - got[3]).max() > 1e-2
    # NULL: bitwise the unmasked entry
    N.check(lib.sd_fbank_lens_f32(plan.handle, x.data_ptr(), B, n, None, out.data_ptr(), 80, ws.data_ptr(), ws.numel(), _stream()), "lens(NULL)")
    assert torch.equal(out, plain)


# ------------------------------------------------------------------ 3. the masked operators against float64

def _masked_stats_f64(x, n_mask, want_std, eps):
    outs = []
    for b, k in enumerate(n_mask):
        xs = x[b, :k]
        m = xs.mean(0)
        outs.append(torch.cat([m, torch.sqrt(((xs - m) ** 2).mean(0).clamp_min(eps))]) if want_std else m)
    return torch.stack(outs)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("B,T,Cc", [(3, 201, 1024), (40, 61, 3072), (2, 626, 512)])
def test_seg_mean_std_lens(dev, dtype, B, T, Cc):
    from speech_diarization_amd.features import length_frames
    N, lib = _lib()
    g = torch.Generator().manual_seed(B * T)
    x = (torch.randn(B * T, Cc, generator=g) * 1.3 + 0.4).to(dtype)
    rel = torch.rand(B, generator=g) * 0.9 + 0.05
    rel[0] = 1.0
    _, n_mask = length_frames(rel, T)
    xd, rd = x.to(dev), rel.to(dev)
    dt = N.SD_DT_F16 if dtype == torch.float16 else N.SD_DT_F32
    for want_std in (0, 1):
        w = 2 * Cc if want_std else Cc
        got = torch.empty(B, w, device=dev)
        N.check(lib.sd_seg_mean_std_lens_dt(xd.data_ptr(), dt, Cc, 0, B, T, rd.data_ptr(), Cc, want_std, C.c_float(1e-12), got.data_ptr(), _stream()), "lens")
        ref = _masked_stats_f64(x.double().view(B, T, Cc), n_mask.tolist(), want_std, 1e-12)
        assert (got.cpu().double() - ref).abs().max() < 2e-5
        plain = torch.empty_like(got)
        N.check(lib.sd_seg_mean_std_dt(xd.data_ptr(), dt, Cc, 0, B, T, Cc, want_std, C.c_float(1e-12), plain.data_ptr(), _stream()), "plain")
        N.check(lib.sd_seg_mean_std_lens_dt(xd.data_ptr(), dt, Cc, 0, B, T, None, Cc, want_std, C.c_float(1e-12), got.data_ptr(), _stream()), "NULL")
        assert torch.equal(got, plain)


def _masked_pool_f64(logits, h, n_mask, eps=1e-12):
    B, T, Cc = h.shape
    mask = torch.arange(T)[None, :, None] < torch.as_tensor(n_mask)[:, None, None]
    a = torch.softmax(logits.masked_fill(~mask, float("-inf")), dim=1)
    mu = (a * h).sum(1)
    sd = torch.sqrt((a * (h - mu[:, None]) ** 2).sum(1).clamp_min(eps))
    return mu, sd


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("B,T,Cc", [(3, 201, 512), (2, 61, 256), (2, 626, 256)])      # LDS kernel (T * 256 B fits), streaming kernel (626)
def test_asp_pool_lens(dev, dtype, B, T, Cc):
    from speech_diarization_amd.features import length_frames
    N, lib = _lib()
    g = torch.Generator().manual_seed(B + T)
    lg = (torch.randn(B * T, Cc, generator=g) * 2).to(dtype)
    h = (torch.randn(B * T, Cc, generator=g) * 1.5 + 0.3).to(dtype)
    rel = torch.tensor([1.0, 0.31, 0.72][:B])
    _, n_mask = length_frames(rel, T)
    dt = N.SD_DT_F16 if dtype == torch.float16 else N.SD_DT_F32
    ld, hd, rd = lg.to(dev), h.to(dev), rel.to(dev)
    got = torch.empty(B, 2 * Cc, device=dev)
    N.check(lib.sd_asp_pool_lens_dt(ld.data_ptr(), Cc, hd.data_ptr(), dt, Cc, B, T, rd.data_ptr(), Cc, C.c_float(1e-12), got.data_ptr(), _stream()), "lens")
    mu, sd = _masked_pool_f64(lg.double().view(B, T, Cc), h.double().view(B, T, Cc), n_mask)
    got = got.cpu().double()
    assert (got[:, :Cc] - mu).abs().max() < 2e-5 and (got[:, Cc:] - sd).abs().max() < 2e-5
    plain = torch.empty(B, 2 * Cc, device=dev)
    again = torch.empty_like(plain)
    N.check(lib.sd_asp_pool_dt(ld.data_ptr(), Cc, hd.data_ptr(), dt, Cc, B, T, Cc, C.c_float(1e-12), plain.data_ptr(), _stream()), "plain")
    N.check(lib.sd_asp_pool_lens_dt(ld.data_ptr(), Cc, hd.data_ptr(), dt, Cc, B, T, None, Cc, C.c_float(1e-12), again.data_ptr(), _stream()), "NULL")
    assert torch.equal(again, plain)


@pytest.mark.parametrize("mode", ["f32", "f16", "split16"])
@pytest.mark.parametrize("B,T,Cc", [(3, 201, 512), (3, 61, 256), (2, 256, 1024), (4, 130, 256), (3, 33, 256)])
def test_asp_attend_pool_lens(dev, mode, B, T, Cc):
    from speech_diarization_amd import ops
    from speech_diarization_amd.features import length_frames
    N, lib = _lib()
    g = torch.Generator().manual_seed(B * 7 + T)
    dtype = torch.float16 if mode == "f16" else torch.float32
    att = 128
    a1 = torch.tanh(torch.randn(B * T, att, generator=g)).to(dtype)
    wc = (torch.randn(Cc, att, 1, generator=g) / 4).to(dtype)
    h = (torch.randn(B * T, Cc, generator=g) * 1.5 + 0.3).to(dtype)
    rel = torch.tensor([0.14, 1.0, 0.63, 0.4][:B])          # row 0: the live frames end inside the first slot / tile
    _, n_mask = length_frames(rel, T)
    wp = ops.pack_weight(wc.float(), dev, dtype)
    dt = {"f32": N.SD_DT_F32, "f16": N.SD_DT_F16, "split16": N.SD_DT_SPLIT16}[mode]
    a1d, hd, rd = a1.to(dev), h.to(dev), rel.to(dev)
    got = torch.empty(B, 2 * Cc, device=dev)
    N.check(lib.sd_asp_attend_pool_lens_dt(a1d.data_ptr(), wp.data_ptr(), hd.data_ptr(), dt, Cc, B, T, rd.data_ptr(), Cc, att,
                                           C.c_float(1e-12), got.data_ptr(), _stream()), "lens")
    logits = (a1.double() @ wc[:, :, 0].double().T).view(B, T, Cc)
    mu, sd = _masked_pool_f64(logits, h.double().view(B, T, Cc), n_mask)
    got = got.cpu().double()
    assert (got[:, :Cc] - mu).abs().max() < 2e-5
    assert (got[:, Cc:] - sd).abs().max() < (2e-4 if mode == "f16" else 2e-5)
    plain = torch.empty(B, 2 * Cc, device=dev)
    again = torch.empty_like(plain)
    N.check(lib.sd_asp_attend_pool_dt(a1d.data_ptr(), wp.data_ptr(), hd.data_ptr(), dt, Cc, B, T, Cc, att, C.c_float(1e-12), plain.data_ptr(),
                                      _stream()), "plain")
    N.check(lib.sd_asp_attend_pool_lens_dt(a1d.data_ptr(), wp.data_ptr(), hd.data_ptr(), dt, Cc, B, T, None, Cc, att, C.c_float(1e-12),
                                           again.data_ptr(), _stream()), "NULL")
    assert torch.equal(again, plain)


# ------------------------------------------------------------------ 4 / 5. the full-geometry forward through encode_batch

def _ragged_batch():
    """8 segments of 0.3 .. 30 s zero-padded to the longest, as embed_segments pads them [REF anti_stick_diarize.py:150-171]."""
    from speech_diarization_amd import synth
    secs = [0.3, 1.0, 2.5, 4.0, 7.5, 12.0, 20.0, 30.0]
    n = int(30.0 * 16000)
    wav = np.zeros((len(secs), n), np.float32)
    lens = np.zeros(len(secs), np.float32)
    for i, s in enumerate(secs):
        k = int(s * 16000)
        wav[i, :k] = synth.synthetic_segments(100 + i, 1, k)[0]
        lens[i] = np.float32(k) / np.float32(n)
    return wav, lens


SHAPES = {
    "B4_n32000": (4, 32000, [1.0, 0.8, 0.55, 0.3]),
    "B3_n9600": (3, 9600, [0.9, 1.0, 0.6]),
    "B3_n100000": (3, 100000, [1.0, 0.45, 0.7]),
}
_REF_CACHE = {}


def _case(name):
    if name not in _REF_CACHE:
        from speech_diarization_amd import synth
        sd = synth.make_ecapa_state_dict(1234)
        if name == "ragged":
            wav, lens = _ragged_batch()
        else:
            B, n, lens = SHAPES[name]
            wav = synth.synthetic_segments(n, B, n)
            lens = np.array(lens, np.float32)
            for b in range(B):
                wav[b, int(np.ceil(lens[b] * n)):] = 0.0
        _REF_CACHE[name] = (sd, wav, lens, R.encode_batch_lens_ref(sd, wav, lens))
    return _REF_CACHE[name]


_ENC = {}


def _encoder(dev, precision, max_batch=512):
    from speech_diarization_amd.speech_encode import HipEcapaEncoder
    key = (precision, max_batch)
    if key not in _ENC:
        sd, _, _, _ = _case("B3_n9600")
        _ENC[key] = HipEcapaEncoder(sd, dev, max_batch=max_batch, precision=precision)
    return _ENC[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["B4_n32000", "B3_n9600", "B3_n100000", "ragged"])
def test_encode_batch_with_wav_lens_matches_float64(dev, precision, name):
    sd, wav, lens, ref = _case(name)
    enc = _encoder(dev, precision)
    x = torch.from_numpy(wav)
    got = enc.encode_batch(x, torch.from_numpy(lens)).squeeze(1).cpu().numpy()
    cd = _cos_dist(got, ref)
    print(f"\n{name} {precision}: max cosine distance to float64 {cd.max():.2e}")
    assert np.isfinite(got).all() and cd.max() < BAR[precision], cd
    # all-ones rel_len through the masked entries: within 1e-6 of the unmasked call (masked reductions instead of colstat)
    ones = torch.ones(wav.shape[0], device=dev)
    xd = x.to(dev)
    masked1 = enc.engine.embed(xd, rel_lens=ones).cpu().numpy()
    plain = enc.encode_batch(x).squeeze(1).cpu().numpy()
    tight = 1e-4 if precision == "f16" else 1e-6          # (f16: the masked squeezes read the f16-rounded activations, colstat its f32 sums)
    assert _cos_dist(masked1, plain).max() < tight
    assert np.array_equal(enc.encode_batch(x, torch.ones(wav.shape[0])).squeeze(1).cpu().numpy(), plain)     # all ones: the same call
    if name == "ragged":
        d = _cos_dist(got, plain)
        assert d[0] > 1e-2 and d[-1] < tight, d                  # the 0.3 s row is no longer 1 % speech; the full row is unchanged


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_encode_batch_with_wav_lens_in_micro_batches(dev, precision):
    sd, wav, lens, ref = _case("ragged")
    got = _encoder(dev, precision, max_batch=3).encode_batch(torch.from_numpy(wav), torch.from_numpy(lens)).squeeze(1).cpu().numpy()
    assert _cos_dist(got, ref).max() < BAR[precision]


# ------------------------------------------------------------------ 6. NaN rows and refused arguments

def test_nan_rows_stay_in_their_row(dev):
    sd, wav, lens, _ = _case("B4_n32000")
    enc = _encoder(dev, "f32")
    base = enc.encode_batch(torch.from_numpy(wav), torch.from_numpy(lens)).squeeze(1).cpu().numpy()
    bad = wav.copy()
    bad[1, 100] = np.nan
    got = enc.encode_batch(torch.from_numpy(bad), torch.from_numpy(lens)).squeeze(1).cpu().numpy()
    assert np.isnan(got[1]).all()
    keep = [0, 2, 3]
    assert np.array_equal(got[keep], base[keep])
    tiny = lens.copy()
    tiny[2] = np.float32(0.4 / 201)                             # p = 0.4: n_norm = 0 (empty sentence mean), n_mask = 1
    got = enc.encode_batch(torch.from_numpy(wav), torch.from_numpy(tiny)).squeeze(1).cpu().numpy()
    assert np.isnan(got[2]).all() and np.isfinite(got[[0, 1, 3]]).all()
    assert np.array_equal(got[[0, 1, 3]], base[[0, 1, 3]])


def test_bad_wav_lens_raise_before_launch(dev):
    _, wav, _, _ = _case("B3_n9600")
    enc = _encoder(dev, "f32")
    x = torch.from_numpy(wav)
    for bad in (torch.ones(2), torch.tensor([0.5, float("nan"), 1.0]), torch.tensor([0.5, 0.0, 1.0]), torch.tensor([1.5, 1.0, 1.0])):
        with pytest.raises(ValueError):
            enc.encode_batch(x, bad)
    with pytest.raises(NotImplementedError):
        enc.encode_batch(x, torch.tensor([0.5, 1.0, 1.0]), normalize=True)


# ------------------------------------------------------------------ 7. pyannote-style masks on ECAPAEncoder

def test_ecapa_encoder_masks_from_the_640_sample_floor(dev):
    """pyannote's mask rule on ECAPAEncoder.  A row is too short (NaN) below the engine's floor, 640 samples = 5 frames: speechbrain's
    reflect padding (k = 3, dil = 4) needs pad < T, so a row keeping 1 mask frame (320 samples) is NaN and one keeping exactly 640
    samples is embedded like every other kept row (earlier the floor was 800 samples and a 640-sample row came back NaN)."""
    from speech_diarization_amd import synth
    from speech_diarization_amd.ecapa_annote import ECAPAEncoder
    enc = ECAPAEncoder(0)
    B, n, F = 5, 32000, 100                                     # 320 samples per mask frame
    w = torch.from_numpy(synth.synthetic_segments(7, B, n))
    plain = enc(w)
    assert torch.equal(enc(w, torch.ones(B, F)), plain)
    masks = torch.zeros(B, F)
    frames = [100, 60, 35, 1, 2]                                # row 3 keeps 320 samples: too short; row 4 keeps 640: the floor
    for b, k in enumerate(frames):
        masks[b, :k] = 1.0
    got = enc(w.unsqueeze(1), masks)
    kept = [k * 320 for k in frames]
    comp = torch.zeros(B, max(kept))
    for b, k in enumerate(kept):
        comp[b, :k] = w[b, :k]
    wl = torch.tensor(kept) / max(kept)
    wl[3] = 1.0
    want = enc.model.encode_batch(comp, wl).squeeze(1)
    ok = [0, 1, 2, 4]
    assert torch.equal(got[ok], want[ok])
    assert torch.isnan(got[3]).all() and torch.isfinite(got[ok]).all()
    short = torch.zeros(B, F)
    short[:, :1] = 1.0
    assert torch.isnan(enc(w, short)).all()
