"""Device route for the voice-activity front: frame scores, hysteresis, opening and closing, speech regions, for many recordings.

`vad.silero_vad_segments` and `diarization_baseline._speech_regions` run the chain frame scores -> `hysteresis_binarize` ->
`morph_open_close` -> `mask_to_segments` on the host, once per recording.  Here the same chain is two launches for a whole folder
(include/sd_hip_vad.h):

* `energy_probs_groups` (`sd_vad_energy_grouped_f32`): the probabilities of `vad.EnergyScorer` for every frame of every recording,
  read from the signal buffer that is on the device already for the embeddings;
* `segments_from_probs_groups` (`sd_vad_segments_grouped`): device probabilities in, region lists out, no host pass.  This is the
  door for a real scorer (Silero on torch-ROCm): whatever made the probabilities, they stay on the device.

What stays on the host is the tail of `mask_to_segments` after its run logic: the padding, the clamp to the signal and its two
rounding regimes, on a few hundred integers per hour of audio (`runs_to_segments`, held equal to `mask_to_segments` by
tests/test_vad_rules.py).  Every parameter the kernel takes is computed here exactly as vad.py computes it.  Everything after the
frame scores is integer-exact; the scores themselves are f64 arithmetic rounded to f32, within a few 1e-7 of the host's f32
(DESIGN.md section 24), so the regions are the host's wherever no probability lies that close to a threshold.

The launches are injectable (`launch=`), as in kmeans_gpu: the CPU tests run the packing and the tail through the numpy statement
of the entries.  There is no implicit CPU route: without a launch, anything that is not a GPU tensor raises.
"""
from __future__ import annotations

import numpy as np
import torch

from . import vad
from .device_rows import DeviceRoute

SHORT, BAD_RANGE, BAD_FRAMES, BAD_CAPACITY, BAD_PROMISE = 1, 2, 4, 8, 16


class DeviceVad(DeviceRoute):
    route, takes = "VAD", "the signal and the probabilities"


def frame_sizes(sr: int, win_ms: float, hop_ms: float) -> tuple[int, int]:
    """(win, hop) in samples, as `vad.frame_audio` rounds them; its ValueError for a hop of no samples."""
    win = int(round(win_ms / 1000.0 * sr))
    hop = int(round(hop_ms / 1000.0 * sr))
    if hop < 1:
        raise ValueError(f"Invalid hop_length: {hop}")
    return win, hop


def frame_counts(n_samples, win: int, hop: int) -> np.ndarray:
    """1 + (n - win) // hop per recording; `vad.frame_audio`'s ValueError for the first recording shorter than a frame."""
    n_samples = np.asarray(n_samples, dtype=np.int64)
    for n in n_samples:
        if n < win:
            raise ValueError(f"Input is too short (n={int(n)}) for frame_length={win}")
    return 1 + (n_samples - win) // hop


def line_lengths(hop_ms: float, open_ms: float, close_ms: float) -> tuple[int, int]:
    """The lengths of `vad.morph_open_close`'s two lines in frames; 1 (the identity) for a stage it skips."""
    return (len(vad._line(open_ms, hop_ms)) if open_ms > 0 else 1), (len(vad._line(close_ms, hop_ms)) if close_ms > 0 else 1)


def run_capacity(n_frames) -> np.ndarray:
    """The runs a mask of n frames can hold, (n + 1) // 2: a recording's share of seg_start / seg_end."""
    return (np.asarray(n_frames, dtype=np.int64) + 1) // 2


def runs_to_segments(seg_start, seg_end, total: int, hop_ms: float, speech_pad_ms: float = 80.0) -> list[tuple[float, float]]:
    """The tail of `vad.mask_to_segments` from its `seg_start` / `seg_end` (frame indices, end exclusive) on: pad, clamp to the
    `total` frames of the mask, and the two rounding regimes [REF vad.py:157-160]."""
    seg_start, seg_end = np.asarray(seg_start, dtype=np.int64), np.asarray(seg_end, dtype=np.int64)
    if seg_start.size == 0:
        return []
    pad = round(speech_pad_ms / hop_ms)
    hop_s = hop_ms / 1000.0
    s = np.round(np.maximum(seg_start - pad, 0) * hop_s, 3)
    e_pad = seg_end + pad
    e = np.round(np.minimum(e_pad, total) * hop_s, 3)
    if e_pad[-1] > total:
        e[e_pad > total] = round(total * hop_s, 3)
    return [(float(a), float(b)) for a, b in zip(s, e)]


def _up(a, dt, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)


def energy_launch(signal, first_sample, n_samples, first_frame, win, hop, threshold_db, slope):
    """The product launch of entry 1: `ops.vad_energy_grouped` on the device of the signal -> (probs, bad), both on the device."""
    from . import ops
    dev = signal.device
    return ops.vad_energy_grouped(signal, _up(first_sample, np.int64, dev), _up(n_samples, np.int32, dev), _up(first_frame, np.int32, dev),
                                  int(first_frame[-1]), win, hop, threshold_db, slope)


def segments_launch(probs, first_frame, first_seg, on, off, open_len, close_len, min_run, max_gap, want_mask):
    """The product launch of entry 2: `ops.vad_segments_grouped` and ONE synchronisation, the copy of its results -> numpy
    (n_segs, seg_start, seg_end, mask or None, bad)."""
    from . import ops
    dev = probs.device
    n_segs, seg_start, seg_end, mask, bad = ops.vad_segments_grouped(probs, _up(first_frame, np.int32, dev), _up(first_seg, np.int32, dev),
                                                                     int(first_seg[-1]), on, off, open_len, close_len, min_run, max_gap,
                                                                     want_mask=want_mask)
    G, cap = n_segs.numel(), seg_start.numel()
    packed = torch.cat([n_segs, bad, seg_start, seg_end]).cpu().numpy()          # one copy for the integers
    n_segs, bad, seg_start, seg_end = np.split(packed, np.cumsum([G, G, cap]))
    return n_segs, seg_start, seg_end, (mask.cpu().numpy() if want_mask else None), bad


def energy_probs_groups(signal_dev, first_sample, n_samples, sr: int = 16000, win_ms: float = 30.0, hop_ms: float = 10.0, scorer=None,
                        launch=None):
    """The frame probabilities `vad.SileroVAD(model=scorer).probs(y_g, sr, win_ms, hop_ms)` of every recording g in one launch, y_g the
    samples [first_sample[g], first_sample[g] + n_samples[g]) of `signal_dev` (f32, 1-d, on the device).  `scorer`: None or a
    `vad.EnergyScorer`, whose two parameters go to the kernel.  -> (probs f32 on the device, first_frame int64 numpy [G + 1]): the
    probabilities of recording g are probs[first_frame[g] : first_frame[g + 1]].  ValueError, before any launch, for a recording
    shorter than a frame (`vad.frame_audio`'s text)."""
    scorer = energy_scorer(scorer)
    win, hop = frame_sizes(sr, win_ms, hop_ms)
    first_sample, n_samples = np.asarray(first_sample, dtype=np.int64), np.asarray(n_samples, dtype=np.int64)
    if first_sample.shape != n_samples.shape or first_sample.ndim != 1 or first_sample.size == 0:
        raise ValueError(f"first_sample and n_samples must be two vectors of one length >= 1, got {first_sample.shape} and {n_samples.shape}")
    first_frame = np.concatenate([[0], np.cumsum(frame_counts(n_samples, win, hop))]).astype(np.int64)
    if np.any(first_sample < 0) or np.any(first_sample + n_samples > int(signal_dev.shape[0])):
        raise ValueError(f"a recording leaves the signal of {int(signal_dev.shape[0])} samples")
    if launch is None:
        DeviceVad.guard(signal_dev)
        launch = energy_launch
    probs, bad = launch(signal_dev, first_sample, n_samples, first_frame, win, hop, float(scorer.threshold_db), float(scorer.slope))
    return probs, first_frame                            # `bad` repeats what was checked above; it is not waited for


def energy_scorer(scorer):
    """The `EnergyScorer` of a device route: the default one for None; any other callable is refused."""
    if scorer is None:
        return vad.EnergyScorer()
    if not isinstance(scorer, vad.EnergyScorer):
        raise ValueError(f"the device VAD scores frames with vad.EnergyScorer only, got {type(scorer).__name__}; score the frames on the "
                         "device yourself and hand the probabilities to vad_gpu.segments_from_probs_groups")
    return scorer


def segments_from_probs_groups(probs_dev, first_frame, hop_ms: float = 10.0, on: float = 0.6, off: float = 0.4, open_ms: float = 80.0,
                               close_ms: float = 40.0, min_speech_ms: float = 250.0, min_gap_ms: float = 100.0, speech_pad_ms: float = 80.0,
                               return_mask: bool = False, launch=None):
    """`vad.mask_to_segments(vad.morph_open_close(vad.hysteresis_binarize(p_g, on, off), hop_ms, open_ms, close_ms), hop_ms,
    min_speech_ms, min_gap_ms, speech_pad_ms)` for every recording g in one launch and one host synchronisation, p_g =
    probs_dev[first_frame[g] : first_frame[g + 1]] (f32 on the device; first_frame: G + 1 non-decreasing integers from 0 to its
    length).  -> one list of (start_s, end_s) per recording; with `return_mask` also the masks after closing, one bool array per
    recording.  ValueError for on <= off: that toggling scan stays on the host (`vad.hysteresis_binarize`)."""
    if not on > off:
        raise ValueError(f"the device VAD needs on > off, got on={on} off={off}; vad.hysteresis_binarize has the literal scan")
    first_frame = np.asarray(first_frame, dtype=np.int64)
    counts = np.diff(first_frame)
    if first_frame.ndim != 1 or first_frame.size < 2 or first_frame[0] != 0 or np.any(counts < 0) or first_frame[-1] != int(probs_dev.shape[0]):
        raise ValueError("first_frame must run from 0 to the number of probabilities without decreasing, one entry more than recordings")
    open_len, close_len = line_lengths(hop_ms, open_ms, close_ms)
    min_run, max_gap = round(min_speech_ms / hop_ms), round(min_gap_ms / hop_ms)
    first_seg = np.concatenate([[0], np.cumsum(run_capacity(counts))]).astype(np.int64)
    if launch is None:
        DeviceVad.guard(probs_dev)
        launch = segments_launch
    n_segs, seg_start, seg_end, mask, bad = launch(probs_dev, first_frame, first_seg, float(on), float(off), open_len, close_len,
                                                   max(int(min_run), 0), max(int(max_gap), 0), bool(return_mask))
    if np.any(bad):
        raise RuntimeError(f"sd_vad_segments_grouped refused recording(s) {np.flatnonzero(bad).tolist()}: flags {bad[bad != 0].tolist()}")
    out = [runs_to_segments(seg_start[q:q + k], seg_end[q:q + k], int(n), hop_ms, speech_pad_ms) for q, k, n in zip(first_seg[:-1], n_segs, counts)]
    if not return_mask:
        return out
    return out, [np.asarray(mask[a:b], dtype=bool) for a, b in zip(first_frame[:-1], first_frame[1:])]


def upload_signals(signals, gap: int = 0, device="cuda"):
    """The recordings concatenated, `gap` zeros after each, uploaded once -> (signal f32 on the device, first_sample, n_samples)."""
    signals = [np.ascontiguousarray(y, dtype=np.float32) for y in signals]
    for y in signals:
        if y.ndim != 1:
            raise ValueError(f"frame_audio expects a 1-D signal, got shape {y.shape}")
    if not torch.cuda.is_available():
        DeviceVad.guard("cpu")
    n_samples = np.array([len(y) for y in signals], dtype=np.int64)
    first_sample = np.concatenate([[0], np.cumsum(n_samples + gap)[:-1]]).astype(np.int64)
    parts = [p for y in signals for p in ((y, np.zeros(gap, np.float32)) if gap else (y,))]
    return torch.from_numpy(np.concatenate(parts)).to(device), first_sample, n_samples


def vad_segments_device(signal_dev, first_sample, n_samples, sr: int = 16000, on_threshold: float = 0.6, off_threshold: float = 0.4,
                        min_speech_ms: float = 250.0, min_silence_ms: float = 100.0, speech_pad_ms: float = 40, win_ms: float = 30.0,
                        hop_ms: float = 10.0, morph_open_ms: float = 80.0, morph_close_ms: float = 40.0, scorer=None):
    """Both launches on a signal that is on the device already -> one region list per recording (see `vad_segments_groups`)."""
    probs, first_frame = energy_probs_groups(signal_dev, first_sample, n_samples, sr, win_ms, hop_ms, scorer)
    return segments_from_probs_groups(probs, first_frame, hop_ms, on_threshold, off_threshold, morph_open_ms, morph_close_ms, min_speech_ms,
                                      min_silence_ms, speech_pad_ms)


def vad_segments_groups(signals, sr: int = 16000, on_threshold: float = 0.6, off_threshold: float = 0.4, min_speech_ms: float = 250.0,
                        min_silence_ms: float = 100.0, speech_pad_ms: float = 40, win_ms: float = 30.0, hop_ms: float = 10.0,
                        morph_open_ms: float = 80.0, morph_close_ms: float = 40.0, scorer=None):
    """`vad.silero_vad_segments(y, sr, ...)` for every recording y of `signals` (1-d float arrays): one upload, two launches, one
    host synchronisation -> one list of (start_s, end_s) per recording.  The frame scorer is `vad.EnergyScorer` (`scorer`: None or
    one with other parameters).  ValueError for a recording shorter than a frame, before any launch."""
    signals = list(signals)
    win, hop = frame_sizes(sr, win_ms, hop_ms)
    frame_counts([np.shape(y)[0] for y in signals if np.ndim(y) == 1], win, hop)          # the host's refusal, before the upload
    energy_scorer(scorer)
    signal, first_sample, n_samples = upload_signals(signals)
    return vad_segments_device(signal, first_sample, n_samples, sr, on_threshold, off_threshold, min_speech_ms, min_silence_ms, speech_pad_ms,
                               win_ms, hop_ms, morph_open_ms, morph_close_ms, scorer)


def vad_segments(y, sr: int = 16000, **kw):
    """`vad.silero_vad_segments(y, sr, **kw)` on the device: `vad_segments_groups` for one recording."""
    return vad_segments_groups([y], sr, **kw)[0]
