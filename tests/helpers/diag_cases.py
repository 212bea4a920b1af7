"""Inputs and doubles shared by the tests of the "VBx-like" diarizer (speech-diarization_amd/diar_diag.py, diag_gpu.py), by
tests/golden/make_diag_golden.py and by tools/time_diag.py: planted low-rank embeddings, a numpy operator for the driver of
diag_gpu, a scripted encoder, scripted frame probabilities and the list of pipeline cases the golden file records.

Imported as a helper (tests/helpers on sys.path)."""
import numpy as np
import torch

D = 192


def planted_lowrank(n, k, r, noise, seed, d=D):
    """k unit centres in R^r; row i = centre[i % k] + noise . N(0, I_r) / sqrt(r), mapped into d dimensions by a random orthonormal
    map, plus a common offset (norm 0.5), times 30, as f32 -> (rows [n, d], labels [n]).

    Low rank on purpose: with whitening, isotropic rows at n <= d make every pair equidistant (the whitened Gram matrix is a
    projector), which gives ties and unstable labels in float64 alone.  The scale 30 puts lambda_max of the covariance far above
    10, where an f32 covariance would be wrong by more than the 1e-6 eigenvalue floor."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, r))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    labels = np.arange(n) % k
    rows = centres[labels] + noise * rng.standard_normal((n, r)) / np.sqrt(r)
    q, _ = np.linalg.qr(rng.standard_normal((d, r)))
    offset = rng.standard_normal(d)
    offset *= 0.5 / np.linalg.norm(offset)
    return ((rows @ q.T + offset) * 30.0).astype(np.float32), labels


# (n, k, r, noise, seed) of the device-against-host comparison of `resegment`
RESEGMENT_CASES = [(48, 3, 6, 0.3, 1), (130, 4, 8, 0.3, 2), (300, 4, 8, 0.4, 3), (1000, 8, 12, 0.4, 4)]


class NumpyDiag:
    """The operator of diag_gpu in numpy f64 over CPU tensors: the statements of include/sd_hip_diag.h, not the kernels' order."""
    device = torch.device("cpu")

    def __init__(self):
        self.calls = []

    def stats(self, X):
        self.calls.append("stats")
        x = X.numpy().astype(np.float64)
        mean = x.sum(0) / x.shape[0]
        xc = x - mean
        return torch.from_numpy(mean), torch.from_numpy(xc.T @ xc)

    def apply(self, X, mean, W):
        self.calls.append("apply")
        v = (X.numpy().astype(np.float64) - mean.numpy()) @ W.numpy()
        return torch.from_numpy((v / (np.linalg.norm(v, axis=1, keepdims=True) + 1e-9)).astype(np.float32))

    def centroids(self, X, labels, k):
        self.calls.append("centroids")
        return centroids_ref(X.numpy(), labels.numpy(), k, 1e-9)


def centroids_ref(x, labels, k, eps_add):
    """sd_label_centroids_f32 in numpy f64, rounded to f32 once -> (centres f32 [k, d], count int32 [k]) as tensors."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros((k, x.shape[1]), np.float32)
    count = np.zeros(k, np.int32)
    for c in range(k):
        rows = x[labels == c]
        count[c] = len(rows)
        if len(rows):
            m = rows.sum(0) / len(rows)
            out[c] = (m / (np.sqrt((m * m).sum()) + eps_add)).astype(np.float32)
    return torch.from_numpy(out), torch.from_numpy(count)


# ------------------------------------------------------------------ the recorded pipeline (tests/golden/diar_diag_pipeline.json)

SR = 16000
CONVERSATION = dict(duration_s=120.0, n_speakers=3, seed=5, turn_s=(1.0, 2.0))
PLANTED = dict(k=3, r=6, noise=0.3, seed=11)


def conversation():
    from speech_diarization_amd import synth
    return synth.synthetic_conversation(sr=SR, **CONVERSATION)


def mask_runs(mask):
    """A boolean mask as run lengths, the first run False (possibly empty)."""
    m = np.asarray(mask, dtype=bool)
    edges = np.flatnonzero(np.diff(np.concatenate(([False], m)).astype(np.int8)))
    return np.diff(np.concatenate(([0], edges, [m.size]))).tolist()


def mask_from_runs(runs):
    return np.repeat(np.arange(len(runs)) % 2 == 1, runs)


def probs_from_segments(segs, n_frames, hop_ms=10.0):
    """Scripted frame probabilities: 0.9 on the frames inside a segment, 0.1 outside."""
    p = np.full(n_frames, 0.1, np.float32)
    for s, e in segs:
        p[int(round(s * 1000.0 / hop_ms)):int(round(e * 1000.0 / hop_ms))] = 0.9
    return p


class ScriptedEncoder:
    """Stand-in for the speaker encoder on both sides: the reference's `SpeakerEncoder.embed(a, sr)` (one piece a call) and the
    repository's `encode_spans(signal, starts, lengths)` (all pieces at once).  The i-th piece gets row i of a planted table, tilted
    by a small deterministic function of its samples (their mean magnitude and their count), so that a piece cut at the wrong
    sample or tiled differently changes its embedding.  `log` holds (length, sum of |samples| as f64) of every piece."""
    sr = SR

    def __init__(self, rows):
        self.rows = np.asarray(rows, np.float32)
        self.log = []

    def _one(self, a):
        a = np.asarray(a, np.float32)
        i = len(self.log)
        self.log.append((int(a.size), float(np.abs(a.astype(np.float64)).sum())))
        tilt = np.float32(1.0 + 1e-3 * np.tanh(float(np.abs(a.astype(np.float64)).mean()) * 10.0) + 1e-9 * (a.size % 1000))
        return (self.rows[i % len(self.rows)] * tilt).astype(np.float32)

    def embed(self, y, sr):
        assert sr == self.sr
        return self._one(y)

    def encode_spans(self, signal, starts, lengths, to_host=True, frame_budget=None):
        signal = np.asarray(signal)
        out = np.stack([self._one(signal[s:s + n]) for s, n in zip(np.asarray(starts).tolist(), np.asarray(lengths).tolist())])
        return out if to_host else torch.from_numpy(out)


def pipeline_cases():
    """name -> keyword arguments of the reference's main beyond its defaults, plus "segs": how the scripted VAD segments are made
    ("turns": the conversation's turns, "turns+short" / "turns+ends": one of them changed by hand) and "rows": "planted" or "scattered"
    (rows that no clusterer groups: every label is noise)."""
    cases = {}
    for cluster in ("agglo", "hdbscan"):
        for whiten in (0, 1):
            for asnorm in (0, 1):
                for use_vbx in (0, 1):
                    # alpha 0.6 where the path is used: at the default 0.995 it never leaves its first state on scores this small
                    cases[f"{cluster}_w{whiten}_a{asnorm}_v{use_vbx}"] = dict(segs="turns", rows="planted", cluster=cluster, whiten=whiten,
                                                                             asnorm=asnorm, use_vbx=use_vbx, **({"alpha": 0.6} if use_vbx else {}))
    # a 0.3 s segment with no context is tiled to 0.4 s; with the default context the first and the last segment are clamped
    cases["tiled_no_context"] = dict(segs="turns+short", rows="planted", cluster="agglo", whiten=0, pad_ctx=0.0)
    cases["clamped_at_both_ends"] = dict(segs="turns+ends", rows="planted", cluster="agglo", whiten=1)
    cases["all_noise"] = dict(segs="turns", rows="scattered", cluster="hdbscan", whiten=0, use_vbx=0)
    return cases


def scripted_segments(kind, turns, duration_s):
    """The speech segments the scripted probabilities stand for, on the 10 ms frame grid."""
    segs = [[round(s, 2), round(e, 2)] for s, e, _ in turns]
    segs = [[s, e] for s, e in segs if e - s >= 0.3]
    if kind == "turns+short":                                        # shorten one turn to 0.3 s: 4800 samples < int(0.4 sr) = 6400
        segs[7][1] = round(segs[7][0] + 0.3, 2)
    elif kind == "turns+ends":                                       # speech from the first frame and up to the last
        segs[0][0] = 0.0
        segs[-1][1] = float(duration_s)
    return segs


def scripted_rows(kind, n):
    if kind == "planted":
        return planted_lowrank(n, d=D, **PLANTED)[0]
    rows = np.zeros((n, D), np.float32)                              # scattered: orthogonal rows, every pair at cosine distance 1
    rows[np.arange(n), np.arange(n)] = 30.0 + np.arange(n)
    return rows
