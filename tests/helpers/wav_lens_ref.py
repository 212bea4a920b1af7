"""float64 reference of speechbrain's relative lengths (`wav_lens`) for the tests.  TEST INFRASTRUCTURE.

PARITY UNPINNED, like the rest of the oracle: speechbrain is not installed, so its code is restated here as it reads in
speechbrain 1.0, statement for statement, and deliberately NOT through the closed forms the library uses
(`features.length_frames`, `sd_norm_frames` / `sd_mask_frames`):

* `InputNormalization(norm_type="sentence", std_norm=False)`:
      actual_size = torch.round(lengths[snt_id] * x.shape[1]).int()
      current_mean = torch.mean(x[snt_id, 0:actual_size, ...], dim=0);  x = x - current_mean
* `length_to_mask(lengths * L, max_len=L)`:  torch.arange(L, dtype=lengths.dtype) < (lengths * L).unsqueeze(1)
* `SEBlock.forward(x, lengths)`:  s = (x * mask).sum(dim=2) / mask.sum(dim=2)
* `AttentiveStatisticsPooling.forward(x, lengths)`:  global context with weights mask / total (population variance, clamp eps),
  attn.masked_fill(mask == 0, -inf), softmax over T, then the same statistics with the attention weights.

The fbank is `oracle.fbank_ref` without its mean (`mean_norm=False`); the network subclasses `oracle.ecapa_ref.EcapaRef`.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.ecapa_ref import ASP_EPS, EcapaRef
from oracle.fbank_ref import fbank_batch_ref, speechbrain_fbank_ref


def sb_actual_sizes(wav_lens, T: int) -> list[int]:
    """InputNormalization's frame count per row, as speechbrain writes it."""
    lengths = torch.as_tensor(wav_lens, dtype=torch.float32).reshape(-1)
    return [int(torch.round(lengths[i] * T).int()) for i in range(lengths.numel())]


def sb_length_to_mask(wav_lens, L: int) -> torch.Tensor:
    """speechbrain's length_to_mask(lengths * L, max_len=L) -> bool [B, L]."""
    lengths = torch.as_tensor(wav_lens, dtype=torch.float32).reshape(-1)
    length = lengths * L
    return torch.arange(L, dtype=length.dtype).expand(len(length), L) < length.unsqueeze(1)


def masked_mean_norm(feats: np.ndarray, wav_lens) -> np.ndarray:
    """[B, T, n_mels] raw (floored) log-mels -> minus each row's mean over its first actual_size frames (float64)."""
    feats = np.asarray(feats, dtype=np.float64)
    out = np.empty_like(feats)
    for b, n in enumerate(sb_actual_sizes(wav_lens, feats.shape[1])):
        with np.errstate(invalid="ignore"):
            mean = feats[b, :n].mean(axis=0) if n > 0 else np.full(feats.shape[2], np.nan)
        out[b] = feats[b] - mean
    return out


def speechbrain_fbank_lens_ref(wavs: np.ndarray, wav_lens) -> np.ndarray:
    """The ECAPA encoder's front end + InputNormalization under wav_lens, float64 -> [B, T, 80]."""
    return masked_mean_norm(speechbrain_fbank_ref(np.asarray(wavs), mean_norm=False), wav_lens)


def torchaudio_fbank_lens_ref(wavs: np.ndarray, wav_lens, sr: int = 16000) -> np.ndarray:
    """fbank_batch's front end (any rate) with the same masked mean, float64 -> [B, T, 80]."""
    return masked_mean_norm(fbank_batch_ref(np.asarray(wavs), sr=sr, mean_nor=False), wav_lens)


class EcapaLensRef(EcapaRef):
    """`EcapaRef` with speechbrain's masked SE squeezes and attentive pooling (`forward_features(feats, wav_lens)`)."""

    def _se_res2net_masked(self, x, i, dilation, mask):
        p = f"blocks.{i}"
        residual = x
        x = self._tdnn(x, f"{p}.tdnn1")
        chunks = torch.chunk(x, self.scale, dim=1)
        ys = []
        for j, c in enumerate(chunks):
            if j == 0:
                y = c
            elif j == 1:
                y = self._tdnn(c, f"{p}.res2net_block.blocks.{j - 1}", dilation)
            else:
                y = self._tdnn(c + y, f"{p}.res2net_block.blocks.{j - 1}", dilation)
            ys.append(y)
        x = torch.cat(ys, dim=1)
        x = self._tdnn(x, f"{p}.tdnn2")
        total = mask.sum(dim=2, keepdim=True)
        s = (x * mask).sum(dim=2, keepdim=True) / total
        s = torch.relu(self._conv(s, f"{p}.se_block.conv1"))
        s = torch.sigmoid(self._conv(s, f"{p}.se_block.conv2"))
        return s * x + residual

    @torch.no_grad()
    def forward_features(self, feats: torch.Tensor, wav_lens=None):
        """feats [B, T, n_mels] (mean-normalised under the same wav_lens) -> [B, emb]."""
        x = feats.to(self.dtype).transpose(1, 2)
        B, _, L = x.shape
        if wav_lens is None:
            wav_lens = torch.ones(B)
        mask = sb_length_to_mask(wav_lens, L).unsqueeze(1).to(self.dtype)     # [B, 1, L]
        x = self._tdnn(x, "blocks.0")
        xl = []
        for i in range(1, self.n_blocks + 1):
            x = self._se_res2net_masked(x, i, i + 1, mask)
            xl.append(x)
        x = self._tdnn(torch.cat(xl, dim=1), "mfa")

        def stats(x, m):
            mean = (m * x).sum(dim=2)
            std = torch.sqrt((m * (x - mean.unsqueeze(2)).pow(2)).sum(dim=2).clamp(ASP_EPS))
            return mean, std

        total = mask.sum(dim=2, keepdim=True)
        mean, std = stats(x, mask / total)
        attn = torch.cat([x, mean.unsqueeze(2).repeat(1, 1, L), std.unsqueeze(2).repeat(1, 1, L)], dim=1)
        attn = self._conv(torch.tanh(self._tdnn(attn, "asp.tdnn")), "asp.conv")
        attn = attn.masked_fill(mask == 0, float("-inf"))
        attn = F.softmax(attn, dim=2)
        mu, sd_ = stats(x, attn)
        pooled = self._bn(torch.cat([mu, sd_], dim=1).unsqueeze(2), "asp_bn")
        return F.conv1d(pooled, self.sd["fc.conv.weight"], self.sd["fc.conv.bias"]).squeeze(2)


def encode_batch_lens_ref(state_dict: dict, wavs: np.ndarray, wav_lens, net: EcapaLensRef | None = None) -> np.ndarray:
    """speechbrain `EncoderClassifier.encode_batch(wavs, wav_lens)` in float64 -> [B, emb]."""
    net = net or EcapaLensRef(state_dict, torch.float64)
    feats = torch.from_numpy(speechbrain_fbank_lens_ref(wavs, wav_lens))
    return net.forward_features(feats, wav_lens).numpy()
