"""No-GPU checks of relative lengths (speechbrain's wav_lens): the host statement of the frame-count rule against speechbrain's
own formulation and hand-made edge cases, the new C-ABI entries, and the argument checks `encode_batch` / `ECAPAEncoder` run
before anything is launched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))

import wav_lens_ref as R  # noqa: E402

from speech_diarization_amd import _native  # noqa: E402
from speech_diarization_amd.features import length_frames  # noqa: E402


def _near(k: float, T: int, steps: int = 12):
    """f32 relative lengths around k / T and the f32 products p = f32(rel * T) they give."""
    r0 = np.float32(k / T)
    rels, r = [r0], r0
    for _ in range(steps):
        r = np.nextafter(r, np.float32(0))
        rels.append(r)
    r = r0
    for _ in range(steps):
        r = np.nextafter(r, np.float32(2))
        rels.append(r)
    rels = np.array([x for x in rels if 0 < x <= 1], np.float32)
    return rels, rels * np.float32(T)


def _check_against_speechbrain(rel, T):
    n_norm, n_mask = length_frames(torch.from_numpy(np.asarray(rel, np.float32)), T)
    assert n_norm.tolist() == R.sb_actual_sizes(rel, T)
    assert n_mask.tolist() == R.sb_length_to_mask(rel, T).sum(1).tolist()
    return n_norm.numpy(), n_mask.numpy()


@pytest.mark.parametrize("T", [61, 200, 201, 626, 3001])
def test_integral_products_and_one_ulp_either_side(T):
    seen = {"exact": 0, "below": 0, "above": 0}
    for k in range(1, T + 1, max(1, T // 37)):
        rels, p = _near(float(k), T)
        n_norm, n_mask = _check_against_speechbrain(rels, T)
        kf = np.float32(k)
        for i in range(len(rels)):
            if p[i] == kf:
                seen["exact"] += 1
                assert (n_norm[i], n_mask[i]) == (k, k)
            elif p[i] == np.nextafter(kf, np.float32(0)):
                seen["below"] += 1
                assert (n_norm[i], n_mask[i]) == (k, k)          # rounds up to k; t < p keeps t = k - 1 as the last frame
            elif p[i] == np.nextafter(kf, np.float32(1e9)):
                seen["above"] += 1
                assert (n_norm[i], n_mask[i]) == (k, min(k + 1, T))   # frame k is (just) inside the mask, not the mean
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("T", [61, 201, 3001])
def test_half_products_round_to_even(T):
    found = 0
    for k in range(0, T - 1, max(1, T // 29)):
        rels, p = _near(k + 0.5, T)
        n_norm, n_mask = _check_against_speechbrain(rels, T)
        for i in np.nonzero(p == np.float32(k + 0.5))[0]:
            found += 1
            assert n_norm[i] == (k if k % 2 == 0 else k + 1)
            assert n_mask[i] == k + 1
    assert found > 0


def test_norm_and_mask_counts_can_differ_by_one():
    n_norm, n_mask = length_frames(torch.tensor([100.3 / 1000.0]), 1000)
    assert (int(n_norm), int(n_mask)) == (100, 101)


def test_tiny_lengths_give_an_empty_mean_and_full_length_gives_T():
    T = 3001
    rel = np.array([1e-6, 0.1 / T, 0.49 / T, 0.51 / T, 1.0], np.float32)
    n_norm, n_mask = _check_against_speechbrain(rel, T)
    assert n_norm.tolist() == [0, 0, 0, 1, T]
    assert n_mask.tolist() == [1, 1, 1, 1, T]


def test_random_lengths_follow_speechbrain():
    g = np.random.default_rng(5)
    for T in (61, 201, 626, 3001):
        rel = np.concatenate([g.uniform(0, 1, 20000), g.integers(1, T + 1, 2000) / T]).astype(np.float32)
        rel = rel[rel > 0]
        _check_against_speechbrain(rel, T)


def test_abi_version_11_exports_the_length_entries():
    lib = _native.load()
    assert _native.SD_ABI_VERSION == 11 and lib.sd_abi_version() == 11
    for name in ("sd_wav_lens_frames", "sd_fbank_lens_f32", "sd_ecapa_forward_lens_f32", "sd_ecapa_forward_lens_f16",
                 "sd_seg_mean_std_lens_dt", "sd_asp_pool_lens_dt", "sd_asp_attend_pool_lens_dt"):
        assert hasattr(lib, name) and name in _native.PROTOTYPES
    # host-side checks, nothing launched
    assert lib.sd_wav_lens_frames(None, 4, 0, None, None, None) == -1
    assert lib.sd_wav_lens_frames(None, 0, 10, None, None, None) == 0
    assert lib.sd_wav_lens_frames(None, 3, 10, None, None, None) == -1 and "no output" in _native.last_error()
    assert lib.sd_fbank_lens_f32(None, None, 1, 16000, None, None, 80, None, 0, None) == -1 and "null plan" in _native.last_error()
    assert lib.sd_ecapa_forward_lens_f32(None, None, 1, 100, None, None, None, 0, None) == -1
    x = (C.c_float * 64)()
    assert lib.sd_asp_attend_pool_lens_dt(C.addressof(x), C.addressof(x), C.addressof(x), _native.SD_DT_F32, 512, 1, 300, None, 512, 128,
                                          1e-12, C.addressof(x), None) == -2                 # T > 256: not covered, nothing launched


def test_encode_batch_argument_checks_need_no_device():
    from speech_diarization_amd.speech_encode import check_wav_lens
    assert check_wav_lens(None, 3) is None
    assert check_wav_lens(torch.ones(3), 3) is None                  # all ones: the unmasked call
    assert check_wav_lens([1, 1], 2) is None
    got = check_wav_lens(torch.tensor([0.5, 1.0, 0.25], dtype=torch.float64), 3)
    assert got.dtype == torch.float32 and got.tolist() == [0.5, 1.0, 0.25]
    for bad, what in [(torch.ones(2), "shape"), (torch.ones(3, 1), "shape"), (torch.tensor([0.5, float("nan"), 1.0]), "finite"),
                      (torch.tensor([0.5, float("inf"), 1.0]), "finite"), (torch.tensor([0.5, 0.0, 1.0]), r"\(0, 1\]"),
                      (torch.tensor([0.5, 1.01, 1.0]), r"\(0, 1\]"), (torch.tensor([-0.5, 1.0, 1.0]), r"\(0, 1\]"),
                      (torch.tensor([True, True, True]), "real")]:
        with pytest.raises(ValueError, match=what):
            check_wav_lens(bad, 3)


def test_pyannote_mask_rule_on_the_host():
    from speech_diarization_amd.ecapa_annote import masked_signals
    n = 4000
    w = torch.arange(3 * n, dtype=torch.float32).reshape(3, n)
    masks = torch.zeros(3, 40)
    masks[0, :40] = 1.0            # everything
    masks[1, 10:30] = 0.9          # the middle half
    masks[2, :3] = 1.0             # 300 samples: too short
    sig, wl, short = masked_signals(w, masks)
    assert sig.shape == (3, n)
    assert torch.equal(sig[0], w[0]) and torch.equal(sig[1, : n // 2], w[1, n // 4: 3 * n // 4]) and not sig[1, n // 2:].any()
    assert torch.equal(sig[2, :300], w[2, :300])
    assert wl.dtype == torch.float32 and wl.tolist() == [1.0, 0.5, 1.0] and short.tolist() == [False, False, True]
    sig, wl, short = masked_signals(w, torch.zeros(3, 40).index_fill_(1, torch.tensor([0, 1]), 1.0))
    assert sig is None and wl is None and short.all()
    with pytest.raises(ValueError):
        masked_signals(w, torch.ones(2, 40))
