"""The shortest segment the embedding path takes, on the host.

Every "same" conv of ECAPA-TDNN pads by reflection (speechbrain's `Conv1d(padding="same", padding_mode="reflect")` calls
`F.pad(mode="reflect")`), which torch accepts for pad < T.  The largest pad is dil * (k - 1) / 2 = 4 (k = 3, dil = 4), so the
network takes T >= 5 frames; with T = 1 + n // 160 that is n >= 640 samples.  Both oracles, the engine and pyannote's mask rule
must agree on that floor."""
import numpy as np
import pytest
import torch

from oracle import ecapa_ref, fbank_ref
from speech_diarization_amd import engine, synth
from speech_diarization_amd.ecapa_annote import MIN_NUM_SAMPLES, masked_signals
from speech_diarization_amd.features import FbankPlan


@pytest.mark.parametrize("cfg", [synth.EcapaConfig(), synth.EcapaConfig.small(64)], ids=["spkrec", "small64"])
def test_floor_is_derived_from_the_geometry(cfg):
    sd = synth.make_ecapa_state_dict(3, cfg)
    got = synth.config_from_state_dict(sd)
    assert engine.min_frames(got) == 5
    assert engine.min_samples(got) == 640
    assert FbankPlan.num_frames(640) == 5 and FbankPlan.num_frames(639) == 4
    assert MIN_NUM_SAMPLES == 640


def test_floor_follows_the_largest_reflect_pad():
    wider = synth.EcapaConfig(kernel_sizes=(5, 3, 3, 5, 1), dilations=(1, 2, 3, 4, 1))       # k = 5, dil = 4: pad 8
    assert engine.min_frames(wider) == 9 and engine.min_samples(wider) == 8 * 160
    stem = synth.EcapaConfig(kernel_sizes=(7, 3, 3, 3, 1), dilations=(1, 1, 1, 1, 1))        # the stem's pad 3 is the largest
    assert engine.min_frames(stem) == 4


def test_mask_rule_floor_is_640_samples():
    n, F = 3200, 100                                       # 32 samples per mask frame
    w = torch.randn(3, n)
    masks = torch.zeros(3, F)
    masks[0, :] = 1.0
    masks[1, :20] = 1.0                                    # 640 samples: long enough
    masks[2, :20] = 1.0
    sig, wl, short = masked_signals(w, masks)
    assert short.tolist() == [False, False, False]
    # 639 kept samples: a mask frame per sample so that the count can be set exactly
    masks = torch.zeros(3, n)
    masks[0, :] = 1.0
    masks[1, :639] = 1.0
    masks[2, :640] = 1.0
    sig, wl, short = masked_signals(w, masks)
    assert short.tolist() == [False, True, False]
    assert wl.tolist() == [1.0, 1.0, np.float32(640 / n)]
    masks[0, 639:] = 0.0
    masks[2, 639:] = 0.0
    sig, wl, short = masked_signals(w, masks)
    assert sig is None and wl is None and short.all()


def test_numpy_oracle_refuses_what_reflect_padding_refuses():
    """`_np_conv` used to reflect twice when pad >= T and return finite values where the torch oracle (F.pad) raises."""
    sd = synth.make_ecapa_state_dict(5, synth.EcapaConfig.small(32))
    feats = np.random.default_rng(0).standard_normal((2, 4, 80))         # T = 4: n = 480..639
    with pytest.raises(ValueError, match="reflect"):
        ecapa_ref.ecapa_forward_numpy(sd, feats)
    with pytest.raises((RuntimeError, ValueError)):
        ecapa_ref.EcapaRef(sd, torch.float64).forward_features(torch.from_numpy(feats))
    x = np.zeros((1, 2, 3))
    w = np.zeros((4, 3, 3))
    with pytest.raises(ValueError):
        ecapa_ref._np_conv(x, w, np.zeros(4), 2)                          # pad 2 >= T 2
    assert ecapa_ref._np_conv(np.ones((1, 3, 3)), w, np.ones(4), 2).shape == (1, 3, 4)


@pytest.mark.parametrize("n", [640, 799])
def test_oracles_agree_at_the_floor(n):
    sd = synth.make_ecapa_state_dict(11, synth.EcapaConfig.small(64))
    wav = synth.synthetic_segments(n, 3, n)
    feats = fbank_ref.speechbrain_fbank_ref(wav)
    assert feats.shape[1] == 1 + n // 160
    a = ecapa_ref.EcapaRef(sd, torch.float64).forward_features(torch.from_numpy(feats)).numpy()
    b = ecapa_ref.ecapa_forward_numpy(sd, feats)
    assert np.isfinite(a).all()
    assert np.abs(a - b).max() < 1e-12 * max(1.0, np.abs(a).max())
