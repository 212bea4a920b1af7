"""The WEIGHT axis without a GPU: the conditions that keep tests/test_gpu_weights.py from being vacuous.  They are conditions on the
generator (tests/helpers/trained_like.py), on the two oracles and on the host packing -- not measurements of the engine.

If a parameter of the generator breaks one of them, the parameter changes, not the condition."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import trained_like as TL  # noqa: E402

CHEAP = [("w128", 2.0), ("w128", 1.0), ("w256a128", 2.0)]
cheap = pytest.mark.parametrize("geom,tail", CHEAP)
CPU_CASES = [c for c in TL.FORWARD_CASES if c[0] != "full"]       # the full width is the GPU module's own fixture (7 s to calibrate)
cpu_cases = pytest.mark.parametrize("geom,tail,B,n", CPU_CASES)


@pytest.fixture(scope="module")
def nets():
    """(geom, tail) -> the trained-like dict, made once per module."""
    made = {}

    def get(geom, tail):
        if (geom, tail) not in made:
            made[geom, tail] = TL.trained_like_state_dict(geom, TL.SEED, tail)
        return made[geom, tail]
    return get


@pytest.fixture(scope="module")
def runs(nets):
    """(geom, tail, B, n) -> (wav, float64 embeddings, its intermediates, float32-oracle embeddings), once per module."""
    from oracle.ecapa_ref import EcapaRef
    from oracle.fbank_ref import speechbrain_fbank_ref
    made = {}

    def get(geom, tail, B, n):
        key = (geom, tail, B, n)
        if key not in made:
            sd, wav = nets(geom, tail), TL.eval_wav(B, n)
            emb, inter = EcapaRef(sd, torch.float64).forward_features(torch.from_numpy(speechbrain_fbank_ref(wav)), return_intermediates=True)
            made[key] = (wav, emb.numpy(), inter, TL.oracle32(sd, wav))
        return made[key]
    return get


# ------------------------------------------------------------------ the generator

def test_two_calls_give_identical_bytes(nets):
    a, b = nets("w128", 2.0), TL.trained_like_state_dict("w128", TL.SEED, 2.0)
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == np.float32 and a[k].tobytes() == b[k].tobytes(), k
    other = TL.trained_like_state_dict("w128", TL.SEED + 1, 2.0)
    assert any(a[k].tobytes() != other[k].tobytes() for k in a)


def _share(n, share):
    return max(1, int(round(share * n)))


@cheap
def test_the_stated_shares_are_present_in_every_tensor(nets, geom, tail):
    sd = nets(geom, tail)
    for key in TL.conv_keys(sd):
        w = sd[key]
        dead = ~np.any(w.reshape(w.shape[0], -1) != 0, axis=1)
        assert int(dead.sum()) == _share(w.shape[0], TL.ZERO_ROWS), key
        if TL.is_frame_level(key):
            b = sd[key[:-len("weight")] + "bias"]                  # N(0, 0.1) +- 3: nothing of the untouched 80 % is past +-2
            assert int((b > 2.0).sum()) == _share(len(b), TL.BIAS_UP) and int((b < -2.0).sum()) == _share(len(b), TL.BIAS_DOWN), key
    for bn in TL.bn_prefixes(sd):
        g = sd[f"{bn}.weight"]                                      # the init draws gamma from [0.5, 1.5)
        assert int((g < 0).sum()) == _share(len(g), TL.NEG_GAMMA), bn
        assert int((np.abs(g) < 2e-3).sum()) == _share(len(g), TL.TINY_GAMMA) and not np.any(g == 0), bn


@cheap
def test_conv_weights_are_heavy_tailed(nets, geom, tail):
    """max / rms of n values cannot exceed sqrt(n), and a 16 x 16 x 3 Res2Net conv has 768: the bar of 50 is held by every tensor that
    could clear it with room, 16384 values (sqrt = 128) and more, at tail 2.0; a Gaussian tensor of that size has 4 to 5.  Every
    tensor, the small ones included, holds 10 (tail 1.0: 12 for the large ones, 5 for all)."""
    sd = nets(geom, tail)
    big, every = (50.0, 10.0) if tail == 2.0 else (12.0, 5.0)
    n_big = 0
    for key in TL.conv_keys(sd):
        w = sd[key].astype(np.float64)
        ratio = np.abs(w).max() / np.sqrt((w ** 2).mean())
        assert ratio >= every, (key, ratio)
        if w.size >= 16384:
            n_big += 1
            assert ratio >= big, (key, ratio)
    assert n_big >= 8


def test_asp_conv_needs_its_own_exponent():
    """Where the fused split pooling runs (w256a128, full), max |w| of asp.conv is past 256: a fixed 2^8 in front of the f16 cast would
    overflow, and at the full width the layer's own s is negative.  (The shape step alone: calibration does not touch conv weights.)"""
    from speech_diarization_amd.engine import split16_exponent
    for geom, s_max in (("w256a128", 1), ("full", -1)):
        w = TL.shaped_state_dict(geom, TL.SEED, 2.0)["asp.conv.conv.weight"]
        assert np.abs(w).max() * 2.0 ** 8 > 65504.0 and split16_exponent(w) <= s_max, (geom, np.abs(w).max())


@cheap
def test_every_batchnorm_holds_the_statistics_of_its_input_on_the_calibration_windows(nets, geom, tail):
    """A float64 forward of the finished dict over the calibration windows: every BatchNorm's input has the recorded mean and the
    recorded variance (floored).  The dict holds f32 roundings (6e-8) of the float64 statistics it was calibrated with, and a later
    layer sees them through at most 40 layers of gain gamma / sqrt(VAR_FLOOR) < 5: 1e-4 of (1 + |statistic|) is far above that and far
    below a statistic taken from another layer or another input."""
    sd = nets(geom, tail)
    net = TL.RecordingRef(sd)
    net.forward_features(TL.calib_feats())
    assert len(net.seen) == len(TL.bn_prefixes(sd))
    for name, (mean, var) in net.seen.items():
        rm, rv = sd[f"{name}.norm.running_mean"].astype(np.float64), sd[f"{name}.norm.running_var"].astype(np.float64)
        assert np.abs(mean - rm).max() <= 1e-4 * (1.0 + np.abs(rm).max()), name
        assert np.abs(np.maximum(var, TL.VAR_FLOOR) - rv).max() <= 1e-4 * (1.0 + np.abs(rv).max()), name
        assert rv.min() >= np.float32(TL.VAR_FLOOR)
    floored = sum(int((sd[f"{bn}.running_var"] == np.float32(TL.VAR_FLOOR)).sum()) for bn in TL.bn_prefixes(sd))
    assert floored > 0                                              # always-off channels exist and sit on the floor


@cpu_cases
def test_evaluation_activations_fit_f16_storage(runs, geom, tail, B, n):
    _, emb, inter, _ = runs(geom, tail, B, n)
    assert np.isfinite(emb).all()
    for name, v in inter.items():
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) < 2.0 ** 11, (name, float(v.abs().max()))


@cpu_cases
def test_some_mfa_channel_is_exactly_constant_over_time(runs, geom, tail, B, n):
    """An always-off channel stores its BatchNorm shift on every frame: the clamp(1e-12) of both standard deviations is reached."""
    h = runs(geom, tail, B, n)[2]["mfa"]
    const = (h.max(dim=2).values == h.min(dim=2).values).all(dim=0)
    assert int(const.sum()) >= 1
    ratio = h.mean(dim=2).abs() / h.std(dim=2, unbiased=False).clamp(min=1e-30)
    assert 0.3 < float(ratio[:, ~const].median()) < 3.0            # |mean| / std of the live channels is about 1, as the issue measured


# ------------------------------------------------------------------ the bars must mean something

@cpu_cases
def test_the_f32_oracle_is_close_and_the_segments_are_apart(runs, geom, tail, B, n):
    _, r64, _, r32 = runs(geom, tail, B, n)
    d_ref32 = TL.cos_dist(r32, r64)
    pairs = [TL.cos_dist(r64[i], r64[j]) for i in range(B) for j in range(i)]
    print(f"\n[{geom} tail {tail} B{B} n{n}] d_ref32 {d_ref32}, pairwise distances {pairs}")
    assert d_ref32.max() <= 1e-9, d_ref32
    assert min(pairs) >= 1e-2, pairs


def test_the_emulated_f16_stores_cost_what_f16_costs(runs, nets):
    """d_emu16 is the yardstick of the f16 bar: it must be an f16-sized error (the init weights sit at 2e-8), neither f32-sized, which
    would mean the subclass rounds nothing, nor a collapsed embedding."""
    for geom, tail, B, n in CPU_CASES:
        wav, r64, _, r32 = runs(geom, tail, B, n)
        d = TL.cos_dist(TL.emu16(nets(geom, tail), wav), r64)
        assert (d > 100.0 * TL.cos_dist(r32, r64)).all() and d.max() < 1e-3, (geom, tail, n, d)


# ------------------------------------------------------------------ the oracle itself

def test_both_oracle_formulations_agree_on_a_trained_like_dict(nets):
    """`ecapa_forward_numpy` had never seen a negative gamma or a zero row."""
    from oracle.ecapa_ref import EcapaRef, ecapa_forward_numpy
    from oracle.fbank_ref import speechbrain_fbank_ref
    for tail in (2.0, 1.0):
        sd = nets("w128", tail)
        feats = speechbrain_fbank_ref(TL.eval_wav(2, 9600))
        a = EcapaRef(sd, torch.float64).forward_features(torch.from_numpy(feats)).numpy()
        b = ecapa_forward_numpy(sd, feats)
        assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max(), np.abs(a - b).max() / np.abs(a).max()


# ------------------------------------------------------------------ packing on the host

def _halves(packed):
    return packed[..., :32].astype(np.float64), packed[..., 32:].astype(np.float64)


@cheap
def test_split16_pack_reconstructs_every_conv_tensor(nets, geom, tail):
    from speech_diarization_amd.engine import pack_conv_weight_split16
    sd = nets(geom, tail)
    subnormal = total = 0
    for key in TL.conv_keys(sd):
        w = sd[key]
        cout, cin, k = w.shape
        packed, s = pack_conv_weight_split16(w)
        hi, lo = _halves(packed)
        v = np.zeros((cout, k, packed.shape[2] * 32))
        v[:, :, :cin] = np.transpose(w.astype(np.float64), (0, 2, 1)) * 2.0 ** s
        top = np.abs(v).max()
        assert 512.0 <= top < 1024.0 and np.isfinite(hi).all() and np.isfinite(lo).all(), (key, s, top)
        rec = (hi + lo).reshape(v.shape)
        assert np.abs(rec - v).max() <= 2.0 ** -22 * top, (key, np.abs(rec - v).max() / top)
        subnormal += int(((lo != 0) & (np.abs(lo) < 2.0 ** -14)).sum())
        total += int((lo != 0).sum())
    print(f"\n[{geom} tail {tail}] {subnormal / total:.1%} of the non-zero low halves are f16 subnormals")
    assert subnormal / total > (0.5 if tail == 2.0 else 0.1)       # the init: under 1 %


def test_split16_pack_of_degenerate_tensors():
    from speech_diarization_amd.engine import pack_conv_weight_split16, split16_exponent
    packed, s = pack_conv_weight_split16(np.zeros((8, 40, 3), np.float32))
    assert s == 0 and not packed.any() and packed.shape == (8, 3, 2, 64)
    for huge in (3.0e4, 1.0e30, 1.0e-30):
        w = np.full((4, 32, 1), 1e-6 * huge / 3.0e4, np.float32)
        w[2, 5, 0] = -huge
        packed, s = pack_conv_weight_split16(w)
        hi, lo = _halves(packed)
        assert s == split16_exponent(w) and np.isfinite(hi).all() and np.isfinite(lo).all()
        assert 512.0 <= -hi[2, 0, 0, 5] < 1024.0 and abs(hi[2, 0, 0, 5] + lo[2, 0, 0, 5] + float(np.float32(huge)) * 2.0 ** s) <= 2.0 ** -22 * 1024.0


@cheap
def test_the_f16_mode_can_hold_this_dict(nets, geom, tail):
    """The f16 mode casts the frame-level weights unscaled: none becomes inf, and `EcapaWeights` takes the dict."""
    from speech_diarization_amd.engine import EcapaWeights
    sd = nets(geom, tail)
    for key in TL.conv_keys(sd):
        if TL.is_frame_level(key):
            assert np.isfinite(sd[key].astype(np.float16)).all(), key
    EcapaWeights(sd, torch.device("cpu"), "f16")


def test_the_f16_mode_refuses_a_weight_it_cannot_hold(nets):
    """A checkpoint may hold a weight past 65504 (f32 does, and the split modes scale it down by their 2^s): the f16 mode must refuse it
    with a ValueError and not upload inf.  The other precisions take the same dict; a per-segment layer (f32 in every mode) may hold it."""
    from speech_diarization_amd.engine import EcapaWeights
    cpu = torch.device("cpu")
    for key in ("blocks.2.tdnn1.conv.conv.weight", "asp.conv.conv.weight", "asp.tdnn.conv.conv.weight"):
        for value in (7.0e4, -65520.0, np.inf):
            sd = dict(nets("w128", 2.0))
            w = sd[key].copy()
            w[3, 2, 0] = value
            sd[key] = w
            with pytest.raises(ValueError, match="f16"):
                EcapaWeights(sd, cpu, "f16")
            if np.isfinite(value):
                for precision in ("f32", "f32s", "f32ns"):
                    EcapaWeights(sd, cpu, precision)
    sd = dict(nets("w128", 2.0))
    w = sd["blocks.1.se_block.conv1.conv.weight"].copy()
    w[3, 2, 0] = 7.0e4
    sd["blocks.1.se_block.conv1.conv.weight"] = w
    EcapaWeights(sd, cpu, "f16")
    w = nets("w128", 2.0)["blocks.2.tdnn1.conv.conv.weight"].copy()
    w[3, 2, 0] = 65519.0                                           # the largest f32 integer that still rounds to 65504
    sd = dict(nets("w128", 2.0))
    sd["blocks.2.tdnn1.conv.conv.weight"] = w
    EcapaWeights(sd, cpu, "f16")


@cheap
def test_rows_without_weights_fold_their_constant_into_the_shift(nets, geom, tail):
    """`fold_constant_rows`: the layer stores the same values (float64: relu(b) s + t), and every row without weights has bias 0, so that
    the column statistics about the shift sum exact zeros for it.  Rows with weights keep their bias, scale and shift bit for bit."""
    from speech_diarization_amd.engine import bn_affine, fold_constant_rows
    sd = nets(geom, tail)
    folded = 0
    for bn in TL.bn_prefixes(sd):
        if bn in ("asp.tdnn.norm.norm", "asp_bn.norm"):
            continue
        conv = bn[:-len(".norm.norm")] + ".conv.conv"
        w, b, (s, t) = sd[f"{conv}.weight"], sd[f"{conv}.bias"], bn_affine(sd, bn)
        b2, (s2, t2) = fold_constant_rows(w, b, (s, t))
        dead = ~np.any(w.reshape(w.shape[0], -1) != 0, axis=1)
        assert dead.any() and not b2[dead].any() and b2.dtype == s2.dtype == t2.dtype == np.float32
        assert np.array_equal(b2[~dead], b[~dead]) and np.array_equal(s2, s) and np.array_equal(t2[~dead], t[~dead])
        want = np.maximum(b[dead].astype(np.float64), 0.0) * s[dead] + t[dead]
        assert np.abs(t2[dead] - want).max() <= 2.0 ** -24 * np.abs(want).max()
        folded += int((b[dead] > 0).sum())
        assert b is sd[f"{conv}.bias"] and np.array_equal(b, sd[f"{conv}.bias"])          # the caller's arrays are not written
    assert folded > 0                                                # some empty row has a positive bias: a non-zero constant behind the ReLU
    w = np.ones((4, 8, 1), np.float32)
    b, aff = np.ones(4, np.float32), (np.ones(4, np.float32), np.ones(4, np.float32))
    out = fold_constant_rows(w, b, aff)
    assert out[0] is b and out[1] is aff


# ------------------------------------------------------------------ the CPU engine path

def test_the_cpu_encoder_of_the_pipeline_test_on_a_trained_like_dict(runs, nets):
    """The encoder tests/test_pipeline_cpu.py injects into the pipeline (the f32 oracle behind `encode_batch_ref`, f32 out)."""
    import test_pipeline_cpu as PC
    for geom, tail, B, n in CPU_CASES[:4]:
        wav, r64, _, r32 = runs(geom, tail, B, n)
        got = PC.cpu_oracle_encoder(sd=nets(geom, tail))(wav)
        assert got.dtype == np.float32 and got.shape == r64.shape
        assert (TL.cos_dist(got, r64) <= 16.0 * TL.cos_dist(r32, r64) + 1e-13).all()
