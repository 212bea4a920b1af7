"""The named entry point: audio file(s) -> (start, end, speaker) segments, RTTM, speaker stems.

Same names, signatures, defaults and output schema as the reference's
`diarization_baseline.py` (`DiarizationParameters` [REF :27-39], `extract_speaker_stems`
[REF :42-160], `merge_same_speaker` [REF :188-213], `adjust_segment_boundaries` [REF :216-233],
`diarize_audio` [REF :236-266], `expand_audios` [REF :273-280], `Diarizer` [REF :283-346],
`main` [REF :349-376]).

`diarize_audio` in the reference drives pyannote's gated `speaker-diarization-3.1` pipeline
(segmentation model + embedding + agglomerative clustering), which cannot be fetched and is
out of scope.  Here the same contract is met by the hot path this repository is about:
VAD -> fixed 2 s windows inside speech -> HIP fbank + ECAPA-TDNN embeddings (one large batch)
-> GPU cosine affinity -> spectral (or AHC) clustering on the host -> per-frame labels ->
turns.  `encoder=` lets BASELINE.json's configs[0] ("PyTorch-CPU ECAPA, plumbing, no GPU")
run the identical plumbing with a CPU encoder; it is never selected implicitly.
"""
from __future__ import annotations

from collections import defaultdict
from dataclasses import dataclass, fields
from pathlib import Path
from typing import Callable

import numpy as np

from . import audio_io, cluster, rttm, vad
from .anti_stick_diarize import cosine_affinity

Encoder = Callable[[np.ndarray], np.ndarray]


@dataclass(frozen=True)
class DiarizationParameters:
    min_stem_s: float = 3.
    max_segment_s: float = 20.0          # longest exported stem
    same_speaker_gap_s: float = 1.2      # neighbouring turns of one speaker merge up to this gap
    max_gap_s: float = 1.5               # silence kept between two pieces of one stem
    fade_ms: float = 20.0                # linear fade at both ends of every piece
    min_speech_duration_s: float = 0.35  # shorter speech is dropped
    min_silence_duration_s: float = 0.1  # shorter silence is bridged
    clustering_threshold: float = 0.7    # cosine similarity threshold for AHC
    min_speakers: int = 2
    max_speakers: int = 6


# ----------------------------------------------------------------------------- segment glue

def merge_same_speaker(segments: list[tuple[float, float, int | str]], max_gap_s: float, max_segment_s: float):
    """Extend a turn with the next one when it is the same speaker, the gap is at most `max_gap_s`
    and the turn built so far is still shorter than `max_segment_s`."""
    merged: list[tuple[float, float, int | str]] = []
    for start, end, spk in segments:
        if merged:
            c_start, c_end, c_spk = merged[-1]
            if c_end - c_start < max_segment_s and spk == c_spk and start - c_end <= max_gap_s:
                merged[-1] = (c_start, max(c_end, end), c_spk)
                continue
        merged.append((start, end, spk))
    return merged


def adjust_segment_boundaries(segments, padding: float) -> list[tuple[float, float, int | str]]:
    """Where two consecutive segments are at least `padding` apart, grow the first's end and pull
    the second's start (not below 0) by `padding` — room for the stems' fades."""
    if len(segments) < 2:
        return segments
    out = list(segments)
    for i in range(len(out) - 1):
        s0, e0, k0 = out[i]
        s1, e1, k1 = out[i + 1]
        if s1 - e0 >= padding:
            out[i] = (s0, e0 + padding, k0)
            out[i + 1] = (max(0, s1 - padding), e1, k1)
    return out


# ----------------------------------------------------------------------------- embedding windows

def speech_windows(speech: list[tuple[float, float]], n_samples: int, sr: int, win_s: float, hop_s: float,
                   margin_s: float = 0.15):
    """Fixed-length windows covering the speech: every `hop_s` inside a region; a region shorter
    than the window gets one window centred on it (shifted to stay inside the signal).
    Returns (start_samples [W], centre_seconds [W], region_index [W])."""
    win = int(round(win_s * sr))
    hop = int(round(hop_s * sr))
    margin = int(round(margin_s * sr))
    starts, regions = [], []
    for r, (s, e) in enumerate(speech):
        a, b = int(round(s * sr)), min(int(round(e * sr)), n_samples)
        if b - a >= win + 2 * margin:      # keep onsets / decays (and the VAD padding) out of the windows
            a, b = a + margin, b - margin
        if b - a >= win:
            st = list(range(a, b - win + 1, hop))
            if st[-1] + win < b:           # cover the tail
                st.append(b - win)
        else:
            mid = (a + b) // 2
            st = [min(max(0, mid - win // 2), max(0, n_samples - win))]
        starts.extend(st)
        regions.extend([r] * len(st))
    starts = np.asarray(starts, dtype=np.int64)
    return starts, (starts + win / 2.0) / sr, np.asarray(regions, dtype=np.int64)


def gather_windows(y: np.ndarray, starts: np.ndarray, win: int) -> np.ndarray:
    """[W, win] float32, zero padded where the signal is shorter than a window."""
    out = np.zeros((len(starts), win), dtype=np.float32)
    for i, s in enumerate(starts):
        piece = y[s: s + win]
        out[i, : len(piece)] = piece
    return out


def labels_to_turns(speech, centres: np.ndarray, regions: np.ndarray, labels: np.ndarray, frame_s: float = 0.01):
    """Inside each speech region every 10 ms frame takes the label of the nearest window centre;
    runs of equal labels become (start, end, label) turns."""
    turns = []
    for r, (s, e) in enumerate(speech):
        sel = np.flatnonzero(regions == r)
        if sel.size == 0:
            continue
        n = max(1, int(round((e - s) / frame_s)))
        t = s + (np.arange(n) + 0.5) * frame_s
        nearest = sel[np.argmin(np.abs(t[:, None] - centres[sel][None, :]), axis=1)]
        lab = labels[nearest]
        cut = np.flatnonzero(np.concatenate(([True], lab[1:] != lab[:-1])))
        ends = np.concatenate((cut[1:], [n]))
        for a, b in zip(cut, ends):
            turns.append((round(s + a * frame_s, 3), round(min(e, s + b * frame_s), 3), int(lab[a])))
    return turns


# ----------------------------------------------------------------------------- the pipeline

def _load(audio) -> tuple[np.ndarray, int, str]:
    if isinstance(audio, dict):
        w = np.asarray(audio["waveform"].cpu().numpy() if hasattr(audio["waveform"], "cpu") else audio["waveform"], dtype=np.float32)
        w = w.mean(axis=0) if w.ndim == 2 else w
        sr = int(audio["sample_rate"])
        if sr != 16000:
            from scipy.signal import resample_poly
            from math import gcd
            g = gcd(sr, 16000)
            w = resample_poly(w, 16000 // g, sr // g).astype(np.float32)
        return np.ascontiguousarray(w), 16000, str(audio.get("uri", "audio"))
    y, sr = audio_io.read_audio(audio, sr=16000, mono=True)
    return y, sr, Path(audio).stem


def diarize_audio(audio_filepath: str | Path | dict, min_speech_duration_s: float, min_silence_duration_s: float,
                  min_speakers: int, max_speakers: int, rttm_filepath: str | Path | None = None, *,
                  encoder: Encoder | None = None, clustering: str = "spectral", clustering_threshold: float = 0.70,
                  window_s: float = 2.0, hop_s: float = 0.25, vad_scorer=None, center_embeddings: bool = True,
                  return_details: bool = False, world: str | None = None,
                  speaker_bounds: bool = False, vad: str = "host", turns: str = "host") -> list[tuple[float, float, str | int]]:
    """-> [(start_s, end_s, "SPEAKER_xx")], RTTM written to `rttm_filepath` when given.

    `world="dist"` (under torchrun, after `dist.init_from_env()`): BASELINE.json configs[2].  Every rank runs the
    host glue on the same audio, embeds only the windows `i mod W == rank` (`dist.shard_indices`), ONE
    `all_gather_into_tensor` returns the full [N, 192] in window order to every rank, every rank clusters
    (deterministic, N x 192 is tiny), rank 0 writes the RTTM.  The result is identical to `world=None`.

    `clustering`: "spectral" (default; eigengap + scikit-learn SpectralClustering on the host), "ahc", "spectral_gpu": the two
    spectral steps on the device (`cluster_gpu`), or "ahc_gpu": the AHC of "ahc" on the device from the rows themselves (`ahc_gpu`; no
    affinity is formed, `details["affinity"]` is None), or "spectral_device": the two steps of "spectral_gpu" with the k-means labels
    from the device too (`cluster_gpu.spectral(..., assign_labels="device")`, `kmeans_gpu`): the same labels wherever the embedding
    has no near-tie.  One recording's ten restarts fill ten of the device's 256 compute units: at 7 609 windows the device labels
    are faster than the host's (the spectral step takes 14.8 ms against 25.9 ms), at 50 000 rows of a 12-column embedding they are
    not (134 ms against 95 to 157 ms for scikit-learn on 16 threads; README, "k-means").  The device routes are HIP path only.

    `speaker_bounds=True` (clustering="ahc_gpu" only; ValueError with any other, since the spectral routes honour the bounds already and
    "ahc" stays the reference's threshold cut): the AHC's cluster count is the threshold's, clamped into [min_speakers, max_speakers]
    (each clamped to the number of windows) by a dendrogram cut on the device (`ahc_gpu`, include/sd_hip_cut.h).

    `vad="device"` (default "host"): the speech regions come from the two launches of `vad_gpu` (include/sd_hip_vad.h) on the signal,
    which is uploaded once and embedded from the same buffer; the same regions wherever no frame probability lies within a few 1e-7
    of a threshold.  `vad_scorer` must then be None or a `vad.EnergyScorer` (ValueError otherwise: hand device probabilities of your
    own to `vad_gpu.segments_from_probs_groups`).  HIP path only.

    `turns="device"` (default "host"), with every `clustering`: relabelling by first appearance and `labels_to_turns` are one upload,
    one launch and one download (`turns_gpu.labels_to_turns_groups`, include/sd_hip_turns.h) instead of a Python loop per window,
    region and run; the same labels and turns, value for value.  HIP path only."""
    _check_speaker_bounds(speaker_bounds, clustering)
    _check_vad(vad, vad_scorer, encoder is None)
    _check_turns(turns, encoder is None)
    y, sr, uri = _load(audio_filepath)
    use_gpu = encoder is None
    if encoder is None:
        from .speech_encode import ecapa_encode_batch
        encoder = ecapa_encode_batch

    y_embed = y                                          # what the windows are read from: the host signal, or its one device copy
    if vad == "device":
        from . import vad_gpu
        vad_gpu.frame_counts([len(y)], *vad_gpu.frame_sizes(sr, 30.0, 10.0))       # the host's refusal of a short recording, before the upload
        y_embed, first_sample, n_samples = vad_gpu.upload_signals([y])
        speech = _speech_regions_device(y_embed, first_sample, n_samples, sr, min_speech_duration_s, min_silence_duration_s, vad_scorer)[0]
    else:
        speech = _speech_regions(y, sr, min_speech_duration_s, min_silence_duration_s, vad_scorer)
    segments: list[tuple[float, float, str | int]] = []
    details = {"speech": speech, "labels": np.zeros(0, dtype=int), "embeddings": np.zeros((0, 192), np.float32)}
    if speech:
        win = int(round(window_s * sr))
        starts, centres, regions = speech_windows(speech, len(y), sr, window_s, hop_s)
        if world is None:
            embs = _embed_windows(encoder, y_embed, starts, win, use_gpu)
        elif world == "dist":
            embs = _embed_sharded(encoder, y_embed, starts, win, use_gpu)
        else:
            raise ValueError(f"world must be None or 'dist', got {world!r}")
        # recording-level mean removal (first step of the reference's whiten_l2, [REF diar_diag.py:187-188]):
        # untrained / mismatched encoders put a large common component into every embedding
        X = cluster.center(embs) if center_embeddings else embs
        if clustering == "ahc_gpu":
            K = None
        else:
            K = _spectral_gpu_affinity(X, use_gpu) if clustering in ("spectral_gpu", "spectral_device") else cosine_affinity(X, use_gpu)
        if clustering == "spectral":
            k = cluster.estimate_num_speakers(K, min_speakers, max_speakers)
            labels = cluster.spectral(K, k)
        elif clustering in ("spectral_gpu", "spectral_device"):
            # the same two steps without the N x N matrix leaving the device (cluster_gpu.py); it is copied out for the details only
            from . import cluster_gpu
            k = cluster_gpu.estimate_num_speakers(K, min_speakers, max_speakers, assume_symmetric=True)
            labels = cluster_gpu.spectral(K, k, assume_symmetric=True, assign_labels="device" if clustering == "spectral_device" else "sklearn")
            K = K.cpu().numpy() if return_details else None
        elif clustering == "ahc":
            labels = cluster.ahc_cosine(K, clustering_threshold)
        elif clustering == "ahc_gpu":
            from . import ahc_gpu
            labels = ahc_gpu.ahc_cosine_rows(_device_rows(X, use_gpu, clustering), clustering_threshold,
                                             **_cluster_bounds(speaker_bounds, min_speakers, max_speakers, [len(X)], one=True))
        else:
            raise ValueError(f"unknown clustering {clustering!r}")
        if turns == "device":
            from . import turns_gpu
            labels, spans = turns_gpu.labels_to_turns_groups([speech], [centres], [regions], [labels])[0]
        else:
            labels = cluster.relabel_by_first_appearance(labels)
            spans = labels_to_turns(speech, centres, regions, labels)
        segments = [(s, e, rttm.speaker_label(k)) for s, e, k in spans]
        details.update(labels=labels, embeddings=embs, affinity=K, window_starts=starts)
    if rttm_filepath and (world is None or _rank() == 0):
        with open(rttm_filepath, "w") as f:
            rttm.write_rttm(segments, uri, f)
    return (segments, details) if return_details else segments


def diarize_audios(audios, min_speech_duration_s: float, min_silence_duration_s: float, min_speakers: int, max_speakers: int,
                   rttm_filepaths=None, *, clustering: str = "ahc_gpu", clustering_threshold: float = 0.70, window_s: float = 2.0,
                   hop_s: float = 0.25, vad_scorer=None, center_embeddings: bool = True, return_details: bool = False,
                   speaker_bounds: bool = False, vad: str = "host", turns: str = "host"):
    """`diarize_audio(..., clustering="ahc_gpu")` for a list of recordings at once -> one segment list per recording (with
    `return_details`: a list of (segments, details)); the RTTM of recording i goes to `rttm_filepaths[i]` when that is given.

    The host glue runs per recording as in `diarize_audio`.  The signals are then uploaded ONCE, concatenated with one window of zeros
    after each (a window that hangs over a recording's end reads zeros, as it does for one recording), and all windows of all
    recordings go through `encode_windows` together: the micro-batches are full whatever the recordings' sizes.  The rows, centred
    per recording, are clustered by ONE driver (`ahc_gpu.ahc_cosine_groups`): one nearest pass and one host synchronisation per
    round for all recordings.  HIP path only, and only clustering="ahc_gpu": the other routes have no grouped form.
    `speaker_bounds=True`: every recording's cluster count is clamped into [min_speakers, max_speakers] as in `diarize_audio`, all
    recordings by one launch of the cut.

    `vad="device"` (default "host"): every recording is uploaded first (the same buffer, one window of zeros after each), the speech
    regions of all of them come from the two launches of `vad_gpu` on that buffer, and the windows are embedded from it: the signal is
    never framed on the host.  `vad_scorer`: None or a `vad.EnergyScorer`, as in `diarize_audio`.

    `turns="device"` (default "host"): after the grouped AHC, the labels of ALL recordings are relabelled and turned into turns by ONE
    call of `turns_gpu.labels_to_turns_groups` (one upload, one launch, one download) instead of a Python loop per recording, region
    and run; `details["labels"]` are the device's relabelled labels.  The same labels and turns, value for value."""
    if clustering != "ahc_gpu":
        raise ValueError(f"diarize_audios clusters all recordings in one driver, which exists for clustering='ahc_gpu' only, got {clustering!r}")
    _check_speaker_bounds(speaker_bounds, clustering)
    _check_vad(vad, vad_scorer, True)
    _check_turns(turns, True)
    audios = list(audios)
    rttm_filepaths = [None] * len(audios) if rttm_filepaths is None else list(rttm_filepaths)
    if len(rttm_filepaths) != len(audios):
        raise ValueError(f"{len(rttm_filepaths)} RTTM paths for {len(audios)} recordings")
    from . import ahc_gpu
    from .speech_encode import using_ecapa_encoder
    sr, win = 16000, int(round(window_s * 16000))
    recs, signal, starts_all, offset = [], [], [], 0
    loaded = [_load(audio) for audio in audios] if vad == "device" and audios else []
    if loaded:
        from . import vad_gpu
        _device_rows(np.zeros((0, 192), np.float32), True, clustering)                 # the refusal without a visible GPU, before any work
        vad_gpu.frame_counts([len(y) for y, _, _ in loaded], *vad_gpu.frame_sizes(sr, 30.0, 10.0))
        signal_dev, first_sample, n_samples = vad_gpu.upload_signals([y for y, _, _ in loaded], gap=win)
        regions_all = _speech_regions_device(signal_dev, first_sample, n_samples, sr, min_speech_duration_s, min_silence_duration_s, vad_scorer)
    for i, audio in enumerate(audios):
        if loaded:
            (y, sr_, uri), speech = loaded[i], regions_all[i]
        else:
            y, sr_, uri = _load(audio)
            speech = _speech_regions(y, sr_, min_speech_duration_s, min_silence_duration_s, vad_scorer)
        starts, centres, regions = speech_windows(speech, len(y), sr, window_s, hop_s) if speech else (np.zeros(0, np.int64), None, None)
        recs.append({"uri": uri, "speech": speech, "starts": starts, "centres": centres, "regions": regions})
        if loaded:                                       # every recording is in the device buffer, at first_sample[i]
            starts_all.append(starts + int(first_sample[i]))
            offset += len(starts)
        elif len(starts):
            signal += [y, np.zeros(win, np.float32)]
            starts_all.append(starts + offset)
            offset += len(y) + win
    sizes = [len(r["starts"]) for r in recs]
    bounds = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    labels = [np.zeros(0, dtype=int)] * len(recs)
    embs = np.zeros((0, 192), np.float32)
    if offset:
        _device_rows(embs, True, clustering)                                            # the refusal without a visible GPU, before any work
        embs = using_ecapa_encoder().encode_windows(signal_dev if loaded else np.concatenate(signal), np.concatenate(starts_all), win)
        X = np.concatenate([cluster.center(embs[a:b]) if center_embeddings and b > a else embs[a:b] for a, b in zip(bounds[:-1], bounds[1:])])
        labels = ahc_gpu.ahc_cosine_groups(_device_rows(X, True, clustering), sizes, clustering_threshold,
                                           **_cluster_bounds(speaker_bounds, min_speakers, max_speakers, sizes))
    out = []
    turned = [None] * len(recs)
    if turns == "device" and offset:                     # ONE launch for the folder
        from . import turns_gpu
        turned = turns_gpu.labels_to_turns_groups([r["speech"] for r in recs], [r["centres"] for r in recs], [r["regions"] for r in recs], labels)
    for r, a, b, lab, path, done in zip(recs, bounds[:-1], bounds[1:], labels, rttm_filepaths, turned):
        segments: list[tuple[float, float, str | int]] = []
        details = {"speech": r["speech"], "labels": np.zeros(0, dtype=int), "embeddings": np.zeros((0, 192), np.float32)}
        if r["speech"]:
            if done is not None:
                lab, spans = done
            else:
                lab = cluster.relabel_by_first_appearance(lab)
                spans = labels_to_turns(r["speech"], r["centres"], r["regions"], lab)
            segments = [(s, e, rttm.speaker_label(k)) for s, e, k in spans]
            details.update(labels=lab, embeddings=embs[a:b], affinity=None, window_starts=r["starts"])
        if path:
            with open(path, "w") as f:
                rttm.write_rttm(segments, r["uri"], f)
        out.append((segments, details) if return_details else segments)
    return out


def _check_speaker_bounds(speaker_bounds: bool, clustering: str) -> None:
    if speaker_bounds and clustering != "ahc_gpu":
        raise ValueError(f"speaker_bounds=True bounds the cluster count of clustering='ahc_gpu'; clustering={clustering!r} "
                         "(the spectral routes honour min_speakers / max_speakers already, 'ahc' is the reference's threshold cut)")


def _cluster_bounds(speaker_bounds: bool, min_speakers: int, max_speakers: int, sizes, one: bool = False) -> dict:
    """The keyword arguments of the `ahc_gpu` drivers: nothing without `speaker_bounds`; otherwise min_speakers and max_speakers, each
    clamped to the number of windows of its recording (at least 1).  1 <= min_speakers <= max_speakers is checked by the driver."""
    if not speaker_bounds:
        return {}
    if not 1 <= int(min_speakers) <= int(max_speakers):
        raise ValueError(f"speaker_bounds=True needs 1 <= min_speakers <= max_speakers, got {min_speakers} and {max_speakers}")
    lo = [max(1, min(int(min_speakers), n)) for n in sizes]
    hi = [max(1, min(int(max_speakers), n)) for n in sizes]
    return {"min_clusters": lo[0] if one else lo, "max_clusters": hi[0] if one else hi}


def _check_vad(vad_route: str, vad_scorer, hip_path: bool) -> None:
    if vad_route not in ("host", "device"):
        raise ValueError(f"vad must be 'host' or 'device', got {vad_route!r}")
    if vad_route == "device":
        from . import vad_gpu
        vad_gpu.energy_scorer(vad_scorer)
        if not hip_path:
            raise RuntimeError("vad='device' runs on the HIP path (no injected encoder, a visible GPU); there is no CPU fallback")


def _check_turns(turns_route: str, hip_path: bool) -> None:
    if turns_route not in ("host", "device"):
        raise ValueError(f"turns must be 'host' or 'device', got {turns_route!r}")
    if turns_route == "device" and not hip_path:
        raise RuntimeError("turns='device' runs on the HIP path (no injected encoder, a visible GPU); there is no CPU fallback")


def _speech_regions_device(signal_dev, first_sample, n_samples, sr: int, min_speech_duration_s: float, min_silence_duration_s: float,
                           vad_scorer=None):
    """`_speech_regions` for every recording of a signal buffer on the device, in the two launches of `vad_gpu` -> one list each."""
    from . import vad_gpu
    return vad_gpu.vad_segments_device(signal_dev, first_sample, n_samples, sr, 0.6, 0.4, min_speech_duration_s * 1000.0,
                                       min_silence_duration_s * 1000.0, 40.0, 30.0, 10.0, 80.0, 40.0, vad_scorer)


def _speech_regions(y: np.ndarray, sr: int, min_speech_duration_s: float, min_silence_duration_s: float, vad_scorer=None):
    """The VAD chain of `diarize_audio`: frame probabilities -> hysteresis -> open / close -> [(start_s, end_s)] speech regions."""
    scorer = vad.SileroVAD(model=vad_scorer or vad.EnergyScorer())
    probs = scorer.probs(y, sr)
    mask = vad.morph_open_close(vad.hysteresis_binarize(probs, 0.6, 0.4), 10.0)
    return vad.mask_to_segments(mask, 10.0, min_speech_ms=min_speech_duration_s * 1000.0,
                                min_gap_ms=min_silence_duration_s * 1000.0, speech_pad_ms=40.0)


def _device_rows(X: np.ndarray, use_gpu: bool, clustering: str):
    """The rows on the device, for the clustering routes that stay there."""
    from .device_rows import upload_rows
    return upload_rows(X, f"clustering={clustering!r} runs on the HIP path (no injected encoder, a visible GPU); there is no CPU fallback",
                       "cuda" if use_gpu else None)


def _spectral_gpu_affinity(X: np.ndarray, use_gpu: bool):
    """`ops.cosine_affinity` of the rows, left on the device for `clustering="spectral_gpu"`."""
    from . import ops
    return ops.cosine_affinity(_device_rows(X, use_gpu, "spectral_gpu"))


def _rank() -> int:
    from . import dist
    return dist.world()[0]


def _embed_windows(encoder: Encoder, y: np.ndarray, starts: np.ndarray, win: int, use_gpu: bool, to_host: bool = True):
    """[len(starts), 192] embeddings of the windows y[s : s + win] (zero padded past the end).  HIP encoder: the signal is
    uploaded ONCE and the fbank kernel reads the windows in place (`sd_fbank_windows_f32`; a 1 h meeting at 2 s / 0.25 s is
    230 MB of signal instead of 1.8 GB of gathered, 8x overlapping windows).  Injected encoder (configs[0], tests): the
    literal host gather the reference's callers do."""
    if use_gpu:
        from .speech_encode import using_ecapa_encoder
        return using_ecapa_encoder().encode_windows(y, starts, win, to_host=to_host)
    return encoder(gather_windows(y, starts, win)) if len(starts) else np.zeros((0, 192), np.float32)


def _embed_sharded(encoder: Encoder, y: np.ndarray, starts: np.ndarray, win: int, use_gpu: bool) -> np.ndarray:
    """Embed this rank's round-robin shard of the windows, all-gather the 192-d rows (RCCL when the process
    group is "nccl": device tensors; gloo: host tensors), return all N rows in window order.  With the HIP encoder
    the embeddings stay on the device from the forward through the collective: one D2H of [N, 192] at the end."""
    import torch
    from . import dist
    rank, w = dist.world()
    n = len(starts)
    mine = dist.shard_indices(n, rank, w)
    on_device = use_gpu and (not torch.distributed.is_initialized() or torch.distributed.get_backend() == "nccl")
    local = _embed_windows(encoder, y, starts[mine], win, use_gpu, to_host=not on_device)
    t = local if isinstance(local, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(local, dtype=np.float32))
    return dist.all_gather_embeddings(t, n).cpu().numpy()


def expand_audios(root: Path):
    if root.is_file():
        root = root.resolve()
        return [root], root.parent
    exts = {".wav", ".flac", ".mp3", ".m4a", ".ogg", ".opus", ".aac"}
    return [p for p in root.rglob("*.*") if p.is_file() and p.suffix.lower() in exts], root


# ----------------------------------------------------------------------------- stems

def plan_speaker_tracks(segments, max_segment_s: float, max_gap_s: float):
    """Per speaker: tracks = lists of ("silence", seconds) / ("speech", start_s, end_s) items, a new
    track starting whenever adding the next turn (plus its leading silence, capped at max_gap_s)
    would exceed max_segment_s [REF diarization_baseline.py:106-153]."""
    per_spk = defaultdict(list)
    for start, end, spk in segments:
        per_spk[spk].append((start, end))
    plans = {}
    for spk, segs in per_spk.items():
        segs.sort()
        tracks, cur, cur_dur, last_end = [], [], 0.0, 0.0
        for i, (s, e) in enumerate(segs):
            sil = min(s - last_end, max_gap_s) if i > 0 else 0.0
            if cur_dur + sil + (e - s) > max_segment_s:
                tracks.append(cur)
                cur, cur_dur, sil = [], 0.0, 0.0
            if sil > 0:
                cur.append(("silence", sil))
                cur_dur += sil
            cur.append(("speech", s, e))
            cur_dur += e - s
            last_end = e
        tracks.append(cur)
        plans[spk] = tracks
    return plans


def extract_speaker_stems(audio: str | Path | dict, segments: list[tuple[float, float, str | int]], root: str | Path,
                          max_segment_s: float, max_gap_s: float, fade_ms: float, min_stem_s: float) -> dict[str | int, list[str]]:
    """One or more stems per speaker under `<root>/<speaker>/<stem>-NNN.flac` (16-bit FLAC, as the reference writes them
    [REF diarization_baseline.py:95-103]; `flac.py`), pieces faded in/out linearly, silences between pieces capped at `max_gap_s`,
    stems shorter than `min_stem_s` skipped."""
    if isinstance(audio, (str, Path)):
        y, sr = audio_io.read_audio(audio, sr=16000, mono=False)
        stem_name = Path(audio).stem
    else:
        y = np.asarray(audio["waveform"], dtype=np.float32)
        y = y[None, :] if y.ndim == 1 else y
        sr = int(audio["sample_rate"])
        stem_name = Path(root).stem
    root = Path(root)
    fade = int(round(fade_ms / 1000.0 * sr))
    ramp = np.linspace(0.0, 1.0, fade, dtype=np.float32) if fade > 0 else None
    out: dict = defaultdict(list)
    for spk, tracks in plan_speaker_tracks(segments, max_segment_s, max_gap_s).items():
        for items in tracks:
            chunks = []
            for it in items:
                if it[0] == "silence":
                    chunks.append(np.zeros((y.shape[0], int(it[1] * sr)), dtype=np.float32))
                else:
                    piece = y[:, int(it[1] * sr): int(it[2] * sr)].copy()
                    if fade > 0 and piece.shape[1] >= 2 * fade:
                        piece[:, :fade] *= ramp
                        piece[:, -fade:] *= ramp[::-1]
                    chunks.append(piece)
            if not chunks:
                continue
            wave = np.concatenate(chunks, axis=1)
            if wave.shape[1] / sr < min_stem_s:
                continue
            path = root / f"{spk}/{stem_name}-{len(out[spk]):03d}.flac"
            path.parent.mkdir(parents=True, exist_ok=True)
            audio_io.write_flac16(path, wave, sr)
            out[spk].append(str(path.absolute()))
    return dict(out)


class Diarizer:
    def __init__(self, hparams: DiarizationParameters, encoder: Encoder | None = None, clustering: str = "spectral",
                 speaker_bounds: bool = False, vad: str = "host", *, turns: str = "host"):
        _check_speaker_bounds(speaker_bounds, clustering)
        _check_vad(vad, None, encoder is None)
        _check_turns(turns, encoder is None)
        self.vad = vad
        self.turns = turns
        self.hparams = hparams
        self.encoder = encoder
        self.clustering = clustering
        self.speaker_bounds = speaker_bounds

    def diarize(self, apath: str | Path | dict, rttm_filepath: str | Path | None):
        hp = self.hparams
        segments = diarize_audio(apath, hp.min_speech_duration_s, min_silence_duration_s=hp.min_silence_duration_s,
                                 min_speakers=hp.min_speakers, max_speakers=hp.max_speakers, rttm_filepath=rttm_filepath,
                                 encoder=self.encoder, clustering=self.clustering,
                                 clustering_threshold=hp.clustering_threshold, speaker_bounds=self.speaker_bounds, vad=self.vad,
                                 turns=self.turns)
        segments = [s for s in segments if s[1] - s[0] >= hp.min_speech_duration_s]
        return sorted(segments)

    def diarize_many(self, apaths, rttm_filepaths=None):
        """`diarize` for a list of recordings through `diarize_audios` (clustering="ahc_gpu", the HIP path): one result per recording."""
        hp = self.hparams
        if self.encoder is not None:
            raise RuntimeError("Diarizer.diarize_many runs on the HIP path (no injected encoder, a visible GPU); there is no CPU fallback")
        many = diarize_audios(apaths, hp.min_speech_duration_s, min_silence_duration_s=hp.min_silence_duration_s,
                              min_speakers=hp.min_speakers, max_speakers=hp.max_speakers, rttm_filepaths=rttm_filepaths,
                              clustering=self.clustering, clustering_threshold=hp.clustering_threshold, speaker_bounds=self.speaker_bounds,
                              vad=self.vad, turns=self.turns)
        return [sorted(s for s in segments if s[1] - s[0] >= hp.min_speech_duration_s) for segments in many]

    def merge_segments(self, segments):
        return merge_same_speaker(segments, self.hparams.same_speaker_gap_s, self.hparams.max_segment_s)

    def pad_segment(self, segments):
        return adjust_segment_boundaries(segments, padding=self.hparams.fade_ms * 2 / 1000)

    def extract_speaker(self, segments, audio_path: str | Path | dict, root: str | Path) -> dict:
        hp = self.hparams
        return extract_speaker_stems(audio_path, segments, root, hp.max_segment_s, hp.max_gap_s, hp.fade_ms, hp.min_stem_s)

    def __call__(self, audio_path: str | Path, root: str | Path, with_rttm: bool = False):
        rttm_filepath = Path(audio_path).with_suffix(".rttm") if with_rttm else None
        segments = self.diarize(audio_path, rttm_filepath)
        segments = self.merge_segments(segments)
        segments = self.pad_segment(segments)
        info = self.extract_speaker(segments, audio_path, root)
        return segments, info


def main(root: str, min_speakers: int = 2, max_speakers: int = 6, max_segment_s: float = 20.0,
         min_silence_duration_s: float = 0.1, min_speech_duration_s: float = 0.35, same_speaker_gap_s: float = 1.,
         max_gap_s: float = 1.5, fade_ms: float = 30.0):
    args = dict(locals())
    args.pop("root")
    unknown = set(args) - {f.name for f in fields(DiarizationParameters)}
    if unknown:                                 # dacite strict=True in the reference
        raise TypeError(f"unknown parameters {sorted(unknown)}")
    hparams = DiarizationParameters(**args)
    diarizer = Diarizer(hparams)
    audios, aroot = expand_audios(Path(root))
    print(aroot, len(audios))
    for apath in audios:
        if apath.with_suffix(".rttm").exists():   # the reference's only resume mechanism
            continue
        troot = apath.with_name(f"{apath.stem}-speakers")
        segments, info = diarizer(apath, troot, True)
        print(apath, len(segments))


if __name__ == "__main__":
    import argparse
    import inspect
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    for name, prm in inspect.signature(main).parameters.items():
        if prm.default is inspect.Parameter.empty:
            ap.add_argument(name)
        else:
            ap.add_argument(f"--{name}", type=type(prm.default), default=prm.default)
    main(**vars(ap.parse_args()))
