"""The reference's "VBx-like" diarizer (`diar_diag.py`): VAD post-processing, one embedding per speech segment with context,
whitening, clustering, cluster centres, AS-norm scores, a Viterbi path, merging and export.

Same function names and semantics as [REF diar_diag.py:25-56, 76-122, 182-208, 213-247, 252-272, 298-433].  Plots are out of scope
(`save_plots` is accepted and ignored), and so are the Silero network (frame probabilities come from `vad.using_silero_vad()`) and
the ERes2NetV2 / CAM++ back ends of `SpeakerEncoder`.

The pipeline is three functions, so that each stage can be tested with doubles and the recording need not be a file:

* `embed_segments_with_context`: the context spans of the segments [REF :341-350] in ONE `encode_spans` call (packed spans: each
  embedded as if alone, as the reference's batch-of-one loop does); pieces shorter than 0.4 s are tiled behind the signal;
* `resegment`: everything from the embeddings to the merged, named segments [REF :352-416].  `device=None` is host arithmetic
  throughout (the reference's numpy); `device="cuda"` keeps every O(N d) array on the GPU: f64 whitening and centres
  (`diag_gpu`, include/sd_hip_diag.h), clustering from the rows (`ahc_gpu`, `hdbscan_gpu`), `ops.asnorm_scores`, `ops.viterbi`;
  labels, the path and the K x d centres are what comes down;
* `diagnose`: the tool's private VAD post-processing on given frame probabilities, then the two stages, then the three files.
`main` is the reference's entry point over them, a plain function.
"""
from __future__ import annotations

import csv
import json
import math
import os

import numpy as np

from .cluster import ahc_cosine, hdbscan_precomputed, whiten_l2  # noqa: F401  (whiten_l2 re-exported)
from .vad import hysteresis_binarize, morph_open_close  # noqa: F401  (the tool's copies [REF :76-96] are the same two scans)


def _l2n(x: np.ndarray) -> np.ndarray:
    return x / (np.linalg.norm(x, axis=-1, keepdims=True) + 1e-9)


def asnorm_scores(query_embs: np.ndarray, ref_centers: np.ndarray, cohort_embs: np.ndarray, topk: int = 200, device=None) -> np.ndarray:
    """Adaptive symmetric score normalisation: cosine scores z-normalised against the top-k cohort
    scores of the query and of the reference, averaged [REF diar_diag.py:196-208].
    `device="cuda"`: the cohort products, the top-k statistics and the combination run on the GPU
    (`ops.asnorm_scores`, f32); default: the reference's numpy arithmetic in the input dtype."""
    if device is not None:
        import torch
        from . import ops
        dev = torch.device(device)
        t = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (query_embs, ref_centers, cohort_embs)]
        return ops.asnorm_scores(t[0], t[1], t[2], topk).cpu().numpy()
    Q, R, Cc = _l2n(np.asarray(query_embs)), _l2n(np.asarray(ref_centers)), _l2n(np.asarray(cohort_embs))
    raw = Q @ R.T
    k = min(topk, Cc.shape[0])
    qc = np.sort(Q @ Cc.T, axis=1)[:, -k:]
    rc = np.sort(R @ Cc.T, axis=1)[:, -k:]
    zq = (raw - qc.mean(axis=1, keepdims=True)) / (qc.std(axis=1, keepdims=True) + 1e-6)
    zr = (raw - rc.mean(axis=1, keepdims=True).T) / (rc.std(axis=1, keepdims=True).T + 1e-6)
    return 0.5 * (zq + zr)


def cluster_embeddings(embs: np.ndarray, method: str = "hdbscan", cos_thr: float = 0.68, affinity=None, clusterer_factory=None) -> np.ndarray:
    """"agglo": average-linkage AHC on 1 - cosine cut at 1 - cos_thr; "hdbscan": HDBSCAN(min_cluster_size=6, min_samples=3,
    metric="precomputed") on 1 - cosine, `allow_single_cluster` left at the clusterer's default [REF diar_diag.py:213-229]
    (`cluster.default_hdbscan_factory` unless `clusterer_factory` is given).  The N x N cosine runs on the GPU
    (`ops.cosine_affinity`) unless `affinity(embs) -> K` is injected (CPU tests)."""
    if method not in ("hdbscan", "agglo"):
        raise ValueError("method must be 'hdbscan' or 'agglo'")
    if affinity is None:
        import torch
        from . import ops
        K = ops.cosine_affinity(torch.from_numpy(np.ascontiguousarray(embs, dtype=np.float32)).cuda()).cpu().numpy()
    else:
        K = np.asarray(affinity(embs))
    if method == "agglo":
        return ahc_cosine(K, cos_thr)
    return hdbscan_precomputed(K, min_cluster_size=6, clusterer_factory=clusterer_factory, min_samples=3, allow_single_cluster=None)


def viterbi_hmm(scores: np.ndarray, alpha: float = 0.995, device=None) -> np.ndarray:
    """Most likely speaker path through per-window log-scores [T, K] under a sticky transition matrix
    (stay alpha, move (1-alpha)/(K-1)), float32 arithmetic as in [REF diar_diag.py:231-247].
    `device="cuda"`: the same recurrence in one wave on the GPU (`ops.viterbi`, K <= 64, f32 scores)."""
    if device is not None:
        import torch
        from . import ops
        sc = torch.from_numpy(np.ascontiguousarray(scores, dtype=np.float32)).to(torch.device(device))
        return ops.viterbi(sc, alpha).cpu().numpy()
    scores = np.asarray(scores)
    T, K = scores.shape
    eps = 1e-8
    logA = np.full((K, K), np.log((1 - alpha) / (K - 1) + eps) if K > 1 else 0.0, dtype=np.float32)
    np.fill_diagonal(logA, np.log(alpha + eps))
    dp = np.full((T, K), -1e9, dtype=np.float32)
    back = np.zeros((T, K), dtype=np.int32)
    dp[0] = scores[0]
    cols = np.arange(K)
    for t in range(1, T):
        cand = dp[t - 1][:, None] + logA
        back[t] = np.argmax(cand, axis=0)
        dp[t] = cand[back[t], cols] + scores[t]
    path = np.zeros(T, dtype=np.int32)
    path[-1] = int(np.argmax(dp[-1]))
    for t in range(T - 2, -1, -1):
        path[t] = back[t + 1, path[t + 1]]
    return path


def save_json(out_path: str, segments: list[dict], speakers: list[str]) -> None:
    with open(out_path, "w", encoding="utf-8") as f:
        json.dump({"segments": segments, "speakers": speakers}, f, ensure_ascii=False, indent=2)


def _srt_time(ts: float) -> str:
    h = int(ts // 3600)
    ts -= h * 3600
    m = int(ts // 60)
    ts -= m * 60
    s = int(ts)
    return f"{h:02d}:{m:02d}:{s:02d},{int(round((ts - s) * 1000)):03d}"


def save_srt(out_path: str, segments: list[dict]) -> None:
    with open(out_path, "w", encoding="utf-8") as f:
        for i, seg in enumerate(segments, 1):
            f.write(f"{i}\n{_srt_time(seg['start'])} --> {_srt_time(seg['end'])}\n{seg['speaker']}\n\n")


def save_csv(out_path: str, segments: list[dict]) -> None:
    with open(out_path, "w", newline="", encoding="utf-8") as f:
        w = csv.DictWriter(f, fieldnames=["start", "end", "speaker"])
        w.writeheader()
        for seg in segments:
            w.writerow({k: seg[k] for k in ("start", "end", "speaker")})


# ----------------------------------------------------------------------------- conditioning and the tool's private VAD post-processing

def load_audio(path: str, sr: int = 16000):
    """-> (mono float32 at `sr`, sr) [REF diar_diag.py:25-34]: read and resampled (`audio_io.read_audio`: WAV / FLAC, polyphase
    resampling where the reference uses librosa's kaiser_fast), mean removed, pre-emphasis 0.97.  librosa is absent, so the
    start state of the pre-emphasis filter is UNPINNED: it is librosa's as recalled (`zi = 2 x[0] - x[1]` handed to `lfilter` as it
    is, i.e. y[0] = 3 x[0] - x[1]), the same restatement as `anti_stick_diarize.diar_read_audio`; only sample 0 depends on it.
    The arithmetic is float64, as on the reference's soundfile array, rounded to float32 at the end."""
    from . import audio_io
    y, s = audio_io.read_audio(path, sr=sr, mono=True)
    y = np.asarray(y, dtype=np.float64)
    if y.size == 0:
        return y.astype(np.float32), s
    y = y - np.mean(y)
    out = np.empty_like(y)
    out[1:] = y[1:] - 0.97 * y[:-1]
    out[0] = y[0] + (2.0 * y[0] - (y[1] if y.size > 1 else y[0]))
    return out.astype(np.float32), s


def loudness_normalize(y: np.ndarray, sr: int, target_lufs: float = -18.0) -> np.ndarray:
    """One gain to `target_lufs` integrated loudness (`loudness.Meter`, BS.1770), then the clip to +-0.99; a signal the meter
    refuses (shorter than one block) is only clipped, as the reference's `except` does [REF diar_diag.py:36-43]."""
    from . import loudness
    try:
        y = loudness.normalize_loudness(y, loudness.Meter(sr).integrated_loudness(y), target_lufs)
    except Exception:
        pass
    return np.clip(y, -0.99, 0.99)


def frame_audio(y: np.ndarray, sr: int, win_ms: float = 30.0, hop_ms: float = 10.0):
    """-> (frames [n, win], hop) with n = 1 + (len - win) // hop; a signal shorter than one window is zero-padded to one
    [REF diar_diag.py:48-56].  (`vad.frame_audio` refuses such a signal and returns the frames alone.)"""
    win = int(round(win_ms / 1000.0 * sr))
    hop = int(round(hop_ms / 1000.0 * sr))
    y = np.asarray(y)
    if len(y) < win:
        y = np.pad(y, (0, win - len(y)))
    return np.lib.stride_tricks.sliding_window_view(y, win)[::hop], hop


def silero_probs_raw(y: np.ndarray, sr: int = 16000, win_ms: float = 30.0, hop_ms: float = 10.0, batch_size: int = 256,
                     device: str = "cpu") -> np.ndarray:
    """Frame probabilities over the tool's own framing [REF diar_diag.py:58-74]; the scorer is `vad.using_silero_vad()`'s (the Silero
    network is a remote download and out of scope), run on the host: 360 k frames an hour."""
    import torch
    from . import vad
    model = vad.using_silero_vad().model
    frames, _ = frame_audio(y, sr, win_ms, hop_ms)
    probs = np.zeros(frames.shape[0], dtype=np.float32)
    with torch.inference_mode():
        for lo in range(0, frames.shape[0], batch_size):
            fb = torch.from_numpy(np.ascontiguousarray(frames[lo:lo + batch_size]))
            probs[lo:lo + fb.shape[0]] = model(fb, sr).float().cpu().numpy()
    return probs


def mask_to_segments(mask: np.ndarray, hop_ms: float, min_speech_ms: float = 250.0, min_gap_ms: float = 100.0) -> list[list[float]]:
    """Boolean frame mask -> [[start_s, end_s]]: runs shorter than `min_speech_ms` dropped, THEN gaps of at most `min_gap_ms`
    bridged [REF diar_diag.py:98-122].  Unlike `vad.mask_to_segments` nothing is padded, clamped or rounded: a time is
    frame index * (hop_ms / 1000) as a float, and the two comparisons are made on those floats, (end - start) * 1000 >= min_speech_ms
    and (start - previous end) * 1000 <= min_gap_ms."""
    m = np.asarray(mask, dtype=bool).reshape(-1)
    hop_s = hop_ms / 1000.0
    edges = np.diff(np.concatenate(([0], m.astype(np.int8), [0])))
    merged: list[list[float]] = []
    for s, e in zip(np.flatnonzero(edges == 1).tolist(), np.flatnonzero(edges == -1).tolist()):
        st, ed = s * hop_s, e * hop_s
        if not (ed - st) * 1000.0 >= min_speech_ms:
            continue
        if merged and (st - merged[-1][1]) * 1000.0 <= min_gap_ms:
            merged[-1][1] = ed
        else:
            merged.append([st, ed])
    return merged


def pad_with_context(y: np.ndarray, sr: int, start: float, end: float, ctx: float = 0.2) -> np.ndarray:
    """y[int((start - ctx) sr) : int((end + ctx) sr)], clamped to the recording [REF diar_diag.py:182-185]."""
    s = max(0, int((start - ctx) * sr))
    e = min(len(y), int((end + ctx) * sr))
    return y[s:e]


# ----------------------------------------------------------------------------- one embedding per segment

def context_spans(segs, n_samples: int, sr: int, pad_ctx: float = 0.2):
    """The samples the reference embeds for every segment [REF diar_diag.py:343-348] -> (starts, lengths, tile_to), int64 [N] each:
    `pad_with_context`'s slice with its `int()` truncations, and for a piece shorter than int(0.4 sr) the length it is tiled to
    (exactly int(0.4 sr); 0 for a piece that is embedded as it is).  An empty piece raises ValueError (the reference divides by 0)."""
    floor = int(0.4 * sr)
    starts, lengths, tile_to = [], [], []
    for st, ed in segs:
        s = max(0, int((st - pad_ctx) * sr))
        e = min(int(n_samples), int((ed + pad_ctx) * sr))
        if e <= s:
            raise ValueError(f"segment [{st}, {ed}] s holds no sample of the {n_samples}-sample recording")
        starts.append(s)
        lengths.append(e - s)
        tile_to.append(floor if e - s < floor else 0)
    return np.asarray(starts, np.int64), np.asarray(lengths, np.int64), np.asarray(tile_to, np.int64)


def embed_segments_with_context(y, sr: int, segs, pad_ctx: float = 0.2, encoder=None, to_host: bool = True):
    """One embedding per segment, each piece embedded as if alone [REF diar_diag.py:341-351] -> [N, D] (numpy, or a tensor on the
    encoder's device with `to_host=False`).  ONE `encoder.encode_spans(signal, starts, lengths, to_host=...)` call: the signal is `y`
    with the tiled short pieces (np.tile(a, ceil(floor / len(a)))[:floor]) appended behind it, so a span either points into `y` or at
    its tiled copy.  encoder: default `speech_encode.using_ecapa_encoder()`; `sr` must be the encoder's rate (the reference's main
    only ever passes 16 kHz; its per-call resampling is not restated)."""
    if encoder is None:
        from .speech_encode import using_ecapa_encoder
        encoder = using_ecapa_encoder()
    y = np.asarray(y, dtype=np.float32)
    starts, lengths, tile_to = context_spans(segs, len(y), sr, pad_ctx)
    tail, at = [], len(y)
    for i in np.flatnonzero(tile_to).tolist():
        a = y[starts[i]:starts[i] + lengths[i]]
        tail.append(np.tile(a, int(math.ceil(tile_to[i] / len(a))))[:tile_to[i]])
        starts[i], lengths[i] = at, tile_to[i]
        at += int(tile_to[i])
    signal = np.concatenate([y] + tail) if tail else y
    return encoder.encode_spans(signal, starts, lengths, to_host=to_host)


# ----------------------------------------------------------------------------- embeddings -> named segments

def merge_segments(segs, labs, gap: float = 0.10) -> list[list]:
    """Consecutive segments of one label whose gap is at most `gap` become one -> [[start, end, label]] [REF diar_diag.py:399-409]."""
    out = []
    cur, s, e = labs[0], segs[0][0], segs[0][1]
    for (st, ed), lb in zip(segs[1:], labs[1:]):
        if lb == cur and st - e <= gap:
            e = ed
        else:
            out.append([s, e, int(cur)])
            cur, s, e = lb, st, ed
    out.append([s, e, int(cur)])
    return out


def _pair_sample(n: int):
    """The reference's sample of segment pairs more than three apart [REF diar_diag.py:361-364]: default_rng(0), two draws."""
    rng = np.random.default_rng(0)
    size = min(2000, n * 4)
    i = rng.integers(0, n, size=size)
    j = rng.integers(0, n, size=size)
    keep = np.abs(i - j) > 3
    return i[keep], j[keep]


def resegment(embs, segs, *, whiten: int = 1, asnorm: int = 1, cluster: str = "hdbscan", cos_thr: float = 0.68, use_vbx: int = 1,
              alpha: float = 0.995, min_gap_ms: float = 100.0, device=None, operator=None, clusterer_factory=None) -> dict:
    """Embeddings [N, D] and their segments [[start, end]] -> the diarization [REF diar_diag.py:352-416], in the reference's order:
    whitening, the two similarity samples, clustering ("hdbscan": min_cluster_size 6, min_samples 3; "agglo": average linkage cut at
    `cos_thr`), the all-noise fallback (one centre over every row), unit centres, scores (AS-norm against the recording's own rows,
    top min(200, N)), the Viterbi path (or the arg-max), `merge_segments(gap=min_gap_ms / 1000)` and the `SPK_i` names.

    -> {"labels": cluster labels int [N], "final_labels": int [N] (indices into the centres), "centers": [K, D], "scores": [N, K],
        "segments": [{"start", "end", "speaker"}] (rounded to 3 decimals), "speakers": sorted names, "adjacent": cosines of
        consecutive rows [N - 1] ([0.0] for one row), "nonadjacent": cosines of the sampled pairs ([0.0] when none)}.

    device=None   host arithmetic throughout: `cluster.whiten_l2`, `cluster_embeddings` over scikit-learn's cosine_similarity
                  (`clusterer_factory` reaches its HDBSCAN slot), the numpy `asnorm_scores` and `viterbi_hmm`; `embs` in its own dtype.
    device="cuda" nothing O(N d) or larger leaves the GPU: `diag_gpu.whiten_l2_rows` (`operator`: its injectable operator),
                  `ahc_gpu.ahc_cosine_rows` / `hdbscan_gpu.hdbscan_rows(6, 3, False, "cosine")`, `ops.label_centroids`,
                  `ops.asnorm_scores`, `ops.viterbi` (the host function above 64 centres), `ops.adjacent_cosine`; f32 rows.  `embs` may
                  be a tensor that is already there; "scores" stays a tensor on the device."""
    if cluster not in ("hdbscan", "agglo"):
        raise ValueError("cluster must be 'hdbscan' or 'agglo'")
    segs = [[float(s), float(e)] for s, e in segs]
    n = len(segs)
    if n == 0 or len(embs) != n:
        raise ValueError(f"{len(embs)} embeddings for {n} segments; at least one segment is needed")
    pi, pj = _pair_sample(n)
    if device is None:
        if operator is not None:
            raise ValueError("operator= belongs to the device route")
        labels, centers, scores, path, adjacent, nonadjacent = _resegment_host(embs, n, pi, pj, whiten, asnorm, cluster, cos_thr, use_vbx,
                                                                               alpha, clusterer_factory)
    else:
        if clusterer_factory is not None:
            raise ValueError("clusterer_factory= belongs to the host route; the device route clusters from the rows")
        labels, centers, scores, path, adjacent, nonadjacent = _resegment_device(embs, n, pi, pj, whiten, asnorm, cluster, cos_thr, use_vbx,
                                                                                 alpha, device, operator)
    uniq = sorted(int(u) for u in np.unique(labels) if u != -1)
    merged = merge_segments(segs, [int(p) for p in path], gap=min_gap_ms / 1000.0)
    spk_map = {k: f"SPK_{i}" for i, k in enumerate(uniq)}
    segments = [{"start": round(s, 3), "end": round(e, 3), "speaker": spk_map.get(lb, f"SPK_{lb}")} for s, e, lb in merged]
    return {"labels": labels, "final_labels": np.asarray(path), "centers": centers, "scores": scores, "segments": segments,
            "speakers": sorted(set(seg["speaker"] for seg in segments)), "adjacent": adjacent, "nonadjacent": nonadjacent}


def _resegment_host(embs, n, pi, pj, whiten, asnorm, cluster, cos_thr, use_vbx, alpha, clusterer_factory):
    from sklearn.metrics.pairwise import cosine_similarity
    embs = np.asarray(embs)
    if whiten:
        embs = whiten_l2(embs)
    unit = embs / np.maximum(np.linalg.norm(embs, axis=1, keepdims=True), np.finfo(embs.dtype).tiny)
    adjacent = np.einsum("ij,ij->i", unit[:-1], unit[1:]) if n > 1 else np.array([0.0])
    nonadjacent = np.einsum("ij,ij->i", unit[pi], unit[pj]) if pi.size else np.array([0.0])
    labels = np.asarray(cluster_embeddings(embs, method=cluster, cos_thr=cos_thr, affinity=cosine_similarity, clusterer_factory=clusterer_factory))
    uniq = sorted(u for u in np.unique(labels) if u != -1)
    if not uniq:                                                     # all noise: one centre over every row [REF :375-377]
        uniq, labels = [0], np.zeros(len(labels), dtype=int)
    centers = []
    for k in uniq:
        m = embs[labels == k].mean(0)
        m /= (np.linalg.norm(m) + 1e-9)
        centers.append(m)
    centers = np.vstack(centers)
    scores = asnorm_scores(embs, centers, embs, topk=min(200, n)) if asnorm else embs @ centers.T
    path = viterbi_hmm(scores, alpha=alpha) if use_vbx else np.argmax(scores, axis=1)
    return labels, centers, scores, path, adjacent, nonadjacent


def _resegment_device(embs, n, pi, pj, whiten, asnorm, cluster, cos_thr, use_vbx, alpha, device, operator):
    import torch
    from . import ahc_gpu, diag_gpu, hdbscan_gpu, ops
    from .device_rows import upload_rows
    X = upload_rows(embs, "resegment(device=...) is the GPU route; there is no CPU fallback (device=None is the host route)", device)
    dev = X.device
    if not bool(torch.isfinite(X).all()):
        raise ValueError("embeddings must be finite")
    if whiten:
        X = diag_gpu.whiten_l2_rows(X, operator=operator)
    adjacent = ops.adjacent_cosine(X).cpu().numpy() if n > 1 else np.array([0.0])
    if pi.size:
        unit = ops.l2norm_rows(X, sklearn_zero_guard=True)
        ti, tj = (torch.from_numpy(v).to(dev) for v in (pi, pj))
        nonadjacent = (unit[ti] * unit[tj]).sum(1).cpu().numpy()    # a gather and a row product over 2000 pairs at most: plumbing
    else:
        nonadjacent = np.array([0.0])
    if cluster == "agglo":
        labels = np.asarray(ahc_gpu.ahc_cosine_rows(X, cos_thr))
    elif n < 3:                                                      # fewer rows than min_samples: all noise, as `hdbscan_precomputed`
        labels = np.full(n, -1, dtype=int)
    else:
        labels = np.asarray(hdbscan_gpu.hdbscan_rows(X, min_cluster_size=6, min_samples=3, allow_single_cluster=False, metric="cosine"))
    uniq = sorted(int(u) for u in np.unique(labels) if u != -1)
    if not uniq:
        uniq, labels = [0], np.zeros(n, dtype=int)
    pos = np.searchsorted(np.asarray(uniq), np.where(labels < 0, uniq[0], labels))
    pos = np.where(labels < 0, -1, pos).astype(np.int32)             # label -> index of its centre, noise stays -1
    centers, _ = diag_gpu.label_centroids_rows(X, torch.from_numpy(pos), len(uniq), operator=operator)
    scores = ops.asnorm_scores(X, centers, X, topk=min(200, n)) if asnorm else ops.rows_product(X, centers)
    if not use_vbx:
        path = torch.argmax(scores, dim=1).cpu().numpy()
    elif len(uniq) <= 64:
        path = ops.viterbi(scores, alpha).cpu().numpy()
    else:
        path = viterbi_hmm(scores.cpu().numpy(), alpha=alpha)
    return labels, centers.cpu().numpy(), scores, path, adjacent, nonadjacent


def save_outputs(out_dir: str, segments: list[dict], speakers: list[str]) -> dict:
    """diarization.json / .srt / .csv in `out_dir` [REF diar_diag.py:417-422] -> their paths."""
    os.makedirs(out_dir, exist_ok=True)
    paths = {k: os.path.join(out_dir, f"diarization.{k}") for k in ("json", "srt", "csv")}
    save_json(paths["json"], segments, speakers)
    save_srt(paths["srt"], segments)
    save_csv(paths["csv"], segments)
    return paths


def diagnose(y, sr: int, probs, *, hop_ms: float = 10.0, vad_on: float = 0.6, vad_off: float = 0.4, open_ms: float = 80.0,
             close_ms: float = 40.0, min_speech_ms: float = 250.0, min_gap_ms: float = 100.0, pad_ctx: float = 0.2, whiten: int = 1,
             asnorm: int = 1, cluster: str = "hdbscan", cos_thr: float = 0.68, use_vbx: int = 1, alpha: float = 0.995, device=None,
             encoder=None, operator=None, clusterer_factory=None, out_dir: str | None = None) -> dict:
    """The conditioned recording `y` and its frame probabilities -> `resegment`'s dict plus "vad_segments" (and "paths" when
    `out_dir` is given: the three files are written there) [REF diar_diag.py:331-422].  ValueError when the VAD leaves no segment."""
    mask = hysteresis_binarize(np.asarray(probs), on=vad_on, off=vad_off)
    mask = morph_open_close(mask, hop_ms, open_ms=open_ms, close_ms=close_ms)
    segs = mask_to_segments(mask, hop_ms, min_speech_ms=min_speech_ms, min_gap_ms=min_gap_ms)
    if not segs:
        raise ValueError("no speech segment found: adjust the VAD thresholds or the open / close lengths")
    embs = embed_segments_with_context(y, sr, segs, pad_ctx=pad_ctx, encoder=encoder, to_host=device is None)
    res = resegment(embs, segs, whiten=whiten, asnorm=asnorm, cluster=cluster, cos_thr=cos_thr, use_vbx=use_vbx, alpha=alpha,
                    min_gap_ms=min_gap_ms, device=device, operator=operator, clusterer_factory=clusterer_factory)
    res["vad_segments"] = segs
    if out_dir is not None:
        res["paths"] = save_outputs(out_dir, res["segments"], res["speakers"])
    return res


def main(audio_path: str, out_dir: str = "out", device: str = "cuda", backend: str = "speechbrain-ecapa", ali_model_id=None,
         vad_on: float = 0.6, vad_off: float = 0.4, win_ms: float = 30.0, hop_ms: float = 10.0, open_ms: float = 80.0,
         close_ms: float = 40.0, min_speech_ms: float = 250.0, min_gap_ms: float = 100.0, pad_ctx: float = 0.2, whiten: int = 1,
         asnorm: int = 1, cluster: str = "hdbscan", cos_thr: float = 0.68, use_vbx: int = 1, alpha: float = 0.995,
         save_plots: int = 1) -> dict:
    """The reference's entry point with its parameter names [REF diar_diag.py:298-433] as a plain function: condition the recording,
    frame probabilities, `diagnose` on `device` (default "cuda": the product route; "cpu" is the host route with the GPU encoder),
    the three files in `out_dir` -> `diagnose`'s dict.  Plots are out of scope: `save_plots` is accepted and ignored.  Only the
    "speechbrain-ecapa" back end exists.  SystemExit(1) when no speech is found, as the reference."""
    if backend != "speechbrain-ecapa":
        raise NotImplementedError(f"backend {backend!r}: only 'speechbrain-ecapa' is built (ERes2NetV2 / CAM++ are out of scope)")
    os.makedirs(out_dir, exist_ok=True)
    y, sr = load_audio(audio_path, sr=16000)
    y = loudness_normalize(y, sr)
    probs = silero_probs_raw(y, sr, win_ms, hop_ms)
    try:
        res = diagnose(y, sr, probs, hop_ms=hop_ms, vad_on=vad_on, vad_off=vad_off, open_ms=open_ms, close_ms=close_ms,
                       min_speech_ms=min_speech_ms, min_gap_ms=min_gap_ms, pad_ctx=pad_ctx, whiten=whiten, asnorm=asnorm, cluster=cluster,
                       cos_thr=cos_thr, use_vbx=use_vbx, alpha=alpha, device=None if str(device) == "cpu" else device, out_dir=out_dir)
    except ValueError as e:
        if "no speech segment" not in str(e):
            raise
        print(str(e))
        raise SystemExit(1)
    adj, non = res["adjacent"], res["nonadjacent"]
    print(f"segments: {len(res['vad_segments'])}  speakers: {res['speakers']}")
    print(f"adjacent cos mean {float(np.mean(adj)):.3f} std {float(np.std(adj)):.3f} | non-adjacent cos mean {float(np.mean(non)):.3f} "
          f"std {float(np.std(non)):.3f}")
    return res
