"""Embedding-model adapters with the reference's class contract [REF ecapa_annote.py:6-33].

The reference subclasses `pyannote.audio.core.model.Model`; pyannote is not part of this
path, so these are plain `torch.nn.Module`s exposing the attributes pyannote's pipeline
reads (`.dimension`, `.forward(waveforms) -> [B, dimension]`).  `forward` also accepts the
`[B, 1, n]` layout pyannote 3.1 hands to its embedding callable, and `__call__(waveforms,
masks=None)` returns what `forward` returns.
"""
from __future__ import annotations

import torch

from .engine import min_samples
from .speech_encode import eres2netv2_encode_batch, using_ecapa_encoder, using_eres2netv2_encoder
from .synth import EcapaConfig


# the engine's shortest segment for the spkrec geometry: ECAPA's reflect padding (k = 3, dil = 4) needs 5 frames = 640 samples;
# ECAPAEncoder uses the floor of the weights it loaded (EmbeddingEngine.min_samples)
MIN_NUM_SAMPLES = min_samples(EcapaConfig())


def masked_signals(waveforms: torch.Tensor, masks: torch.Tensor, min_num_samples: int = MIN_NUM_SAMPLES):
    """pyannote 3.x's rule for a speechbrain embedding under frame masks: (signals [B, max_kept], wav_lens f32 [B], too_short bool [B]),
    or (None, None, too_short) when every row keeps fewer than `min_num_samples` samples.
      1. imask = nearest-interpolate(masks, num_samples) > 0.5;
      2. the kept samples of each row in order, zero-padded to the longest kept row;
      3. wav_lens = kept / max_kept (f32);
      4. rows keeping fewer than min_num_samples samples get wav_lens = 1 (their embedding is to be replaced by NaN)."""
    B, n = waveforms.shape
    if masks.dim() != 2 or masks.shape[0] != B:
        raise ValueError(f"masks must be [{B}, num_frames], got {tuple(masks.shape)}")
    imasks = torch.nn.functional.interpolate(masks.float().unsqueeze(1), size=n, mode="nearest").squeeze(1) > 0.5
    imasks = imasks.to(waveforms.device)
    kept = imasks.sum(dim=1)
    too_short = kept < min_num_samples
    max_kept = int(kept.max())
    if max_kept < min_num_samples:
        return None, None, too_short
    signals = torch.nn.utils.rnn.pad_sequence([w[m] for w, m in zip(waveforms, imasks)], batch_first=True)
    wav_lens = (kept / max_kept).to(torch.float32)
    wav_lens[too_short] = 1.0
    return signals, wav_lens, too_short


class ECAPAEncoder(torch.nn.Module):
    def __init__(self, device: str | int = 0):
        super().__init__()
        self.model = using_ecapa_encoder(device)
        self.dimension = 192  # [REF ecapa_annote.py:11]
        self.sample_rate = 16000

    def forward(self, waveforms: torch.Tensor, masks: torch.Tensor | None = None) -> torch.Tensor:
        """waveforms: (batch, num_samples) or (batch, 1, num_samples) -> (batch, dimension),
        on the encoder's device [REF ecapa_annote.py:13-22].  masks (batch, num_frames), optional: pyannote's frame
        weights; the kept samples of each row are compacted and embedded with relative lengths (`masked_signals`),
        rows keeping fewer samples than the engine's shortest segment (`EmbeddingEngine.min_samples`: 640 = 5 frames for the
        spkrec geometry) come back as NaN.  None or all ones: the unmasked call."""
        if waveforms.dim() == 3:
            if waveforms.shape[1] != 1:
                raise ValueError("expected mono waveforms [B, 1, n]")
            waveforms = waveforms[:, 0, :]
        if masks is None or bool(torch.all(masks == 1)):
            return self.model.encode_batch(waveforms).squeeze(1)
        signals, wav_lens, too_short = masked_signals(waveforms, masks, self.model.engine.min_samples)
        if signals is None:                  # every row too short: no launch
            return torch.full((waveforms.shape[0], self.dimension), float("nan"), device=self.model.device)
        emb = self.model.encode_batch(signals, wav_lens).squeeze(1)
        return emb.masked_fill(too_short.to(emb.device).unsqueeze(1), float("nan"))


class ERes2NetV2Encoder(torch.nn.Module):
    """Kept for interface parity [REF ecapa_annote.py:25-33]; constructing it fails like the reference
    does without its ONNX file (the ERes2NetV2 network is outside this hot path)."""

    def __init__(self, device: str | int = 0):
        super().__init__()
        self.model = using_eres2netv2_encoder()
        self.dimension = 192

    def forward(self, waveforms: torch.Tensor) -> torch.Tensor:
        y = eres2netv2_encode_batch(waveforms.cpu().numpy())
        return torch.from_numpy(y).to(waveforms.device)
