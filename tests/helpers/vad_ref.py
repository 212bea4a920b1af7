"""The numpy statement of the two entries of include/sd_hip_vad.h, the run form of the morphology they use, and the inputs the VAD tests
share.

* `energy_probs64`: entry 1 in float64, frame by frame: what the device is held to (and what the host's f32 `EnergyScorer` is
  measured against).
* `hysteresis`, `keep_long`, `join_near`, `clip`: the stages of entry 2 on run lists; `segments_entry` is the entry (n_segs,
  seg_start, seg_end, mask, bad for many recordings), `runs_of` / `mask_of` convert.
* tests/test_vad_rules.py holds these equal to scipy.ndimage and to vad.py; tests/test_gpu_vad.py holds the device equal to these.
"""
import numpy as np

SHORT, BAD_RANGE, BAD_FRAMES, BAD_CAPACITY, BAD_PROMISE = 1, 2, 4, 8, 16
LDS_FRAMES = 16383
LINES = (1, 2, 3, 4, 5, 8, 9)
BAND = 1e-4

# (open_len, close_len, min_run, max_gap): diarize_audio's, anti_stick's, hop 12.5 ms, an odd opening, the identity stages
PARAMS = {"diarize_audio": (8, 4, 35, 10), "anti_stick": (8, 4, 25, 10), "hop12.5": (6, 3, 20, 8), "odd_open": (5, 4, 35, 10),
          "identity": (1, 1, 0, 0)}


# ------------------------------------------------------------------ entry 1

def energy_probs64(y, win: int, hop: int, threshold_db: float = -35.0, slope: float = 0.6) -> np.ndarray:
    """float64 [1 + (len(y) - win) // hop]: mean of squares, clamp at 1e-12, sqrt, 20 log10, logistic; a NaN stays a NaN."""
    y = np.asarray(y, dtype=np.float32).astype(np.float64)
    frames = np.lib.stride_tricks.sliding_window_view(y, win)[::hop]
    with np.errstate(over="ignore", invalid="ignore"):
        m = (frames * frames).sum(axis=1) / win
        m = np.where(m < 1e-12, 1e-12, m)
        z = slope * (20.0 * np.log10(np.sqrt(m)) - threshold_db)
        return 1.0 / (1.0 + np.exp(-z))


def frame_count(n: int, win: int, hop: int) -> int:
    return 1 + (n - win) // hop if n >= win else 0


def energy_entry(signal, first_sample, n_samples, first_frame, win, hop, threshold_db=-35.0, slope=0.6):
    """Entry 1 with its flags -> (probs f64 [n_frames], bad int32 [G]): NaN for every frame of a bad recording and for frames that
    belong to none."""
    G, n_frames = len(n_samples), int(first_frame[-1])
    probs, bad = np.full(n_frames, np.nan), np.zeros(G, np.int32)
    for g in range(G):
        ns, fs, lo, hi = int(n_samples[g]), int(first_sample[g]), int(first_frame[g]), int(first_frame[g + 1])
        bits = (SHORT if ns < win else 0) | (BAD_RANGE if ns < 0 or fs < 0 or fs + ns > len(signal) else 0)
        if lo < 0 or hi > n_frames or hi - lo != frame_count(ns, win, hop) or (g == 0 and lo != 0) or (g == G - 1 and hi != n_frames):
            bits |= BAD_FRAMES
        bad[g] = bits
    for g in range(G):                                   # a frame belongs to the LAST recording that starts at or before it
        if bad[g] == 0:
            lo, hi = int(first_frame[g]), int(first_frame[g + 1])
            own = [f for f in range(lo, hi) if max(i for i in range(G) if i == 0 or first_frame[i] <= f) == g]
            p = energy_probs64(signal[first_sample[g]:first_sample[g] + n_samples[g]], win, hop, threshold_db, slope)
            for f in own:
                probs[f] = p[f - lo]
    return probs, bad


# ------------------------------------------------------------------ entry 2, stage by stage

def hysteresis(p, on, off) -> np.ndarray:
    """bool [n]: the most recent event at or before i is a start (p >= on); p < off is a stop; compared in f32."""
    p = np.asarray(p, dtype=np.float32)
    on, off = np.float32(on), np.float32(off)
    assert on > off
    with np.errstate(invalid="ignore"):
        event = np.where(p >= on, 1, np.where(p < off, 2, 0))
    last = np.maximum.accumulate(np.where(event != 0, np.arange(len(p)), -1)) if len(p) else np.zeros(0, int)
    return (last >= 0) & (event[np.maximum(last, 0)] == 1)


def hysteresis_literal(p, on, off) -> np.ndarray:
    """The same by the scan itself, frame after frame"""
    p = np.asarray(p, dtype=np.float32)
    on, off = np.float32(on), np.float32(off)
    out, state = np.zeros(len(p), bool), False
    for i, v in enumerate(p):
        if v >= on:
            state = True
        elif v < off:
            state = False
        out[i] = state
    return out


def runs_of(mask):
    """[(start, end)] of the runs of True, end exclusive"""
    edges = np.diff(np.concatenate(([0], np.asarray(mask, dtype=np.int8), [0])))
    return list(zip(np.flatnonzero(edges == 1).tolist(), np.flatnonzero(edges == -1).tolist()))


def mask_of(runs, n) -> np.ndarray:
    out = np.zeros(n, bool)
    for s, e in runs:
        out[s:e] = True
    return out


def keep_long(runs, min_len):
    return [(s, e) for s, e in runs if e - s >= min_len]


def join_near(runs, max_gap):
    out = []
    for s, e in runs:
        if out and s - out[-1][1] <= max_gap:
            out[-1] = (out[-1][0], e)
        else:
            out.append((s, e))
    return out


def clip(runs, lo, hi):
    return [(max(s, lo), min(e, hi)) for s, e in runs if min(e, hi) > max(s, lo)]


def opening(runs, L):
    """scipy.ndimage.binary_opening with a line of L: the runs of at least L frames"""
    return keep_long(runs, L)


def closing(runs, L, n):
    """scipy.ndimage.binary_closing with a line of L on n frames: gaps shorter than L filled, then the first L // 2 and the last
    L - 1 - L // 2 frames cleared"""
    c = L // 2
    return clip(join_near(runs, L - 1), c, n - (L - 1 - c))


def stages(p, on, off, open_len, close_len, min_run, max_gap):
    """-> (run lists after hysteresis, opening, closing, the short-run rule, the gap rule): every count the capacity bound speaks of"""
    n = len(p)
    r0 = runs_of(hysteresis(p, on, off))
    r1 = opening(r0, open_len)
    r2 = closing(r1, close_len, n)
    r3 = keep_long(r2, min_run)
    r4 = join_near(r3, max_gap)
    return r0, r1, r2, r3, r4


def segments_entry(probs, first_frame, first_seg, on, off, open_len, close_len, min_run, max_gap, seg_fill=-1):
    """Entry 2 -> (n_segs [G], seg_start [seg_cap], seg_end [seg_cap], mask uint8 [n_frames], bad [G]); what the entry leaves alone
    holds `seg_fill`."""
    first_frame, first_seg = np.asarray(first_frame, np.int64), np.asarray(first_seg, np.int64)
    G, n_frames, seg_cap = len(first_frame) - 1, len(probs), int(first_seg[-1]) if len(first_seg) else 0
    n_segs, bad = np.zeros(G, np.int32), np.zeros(G, np.int32)
    seg_start, seg_end = np.full(seg_cap, seg_fill, np.int32), np.full(seg_cap, seg_fill, np.int32)
    mask = np.zeros(n_frames, np.uint8)
    return _segments_fill(probs, first_frame, first_seg, G, n_frames, seg_cap, (on, off, open_len, close_len, min_run, max_gap), n_segs, seg_start,
                          seg_end, mask, bad)


def promise_broken(table, last) -> bool:
    table = np.asarray(table, np.int64)
    return bool(table[0] != 0 or table[-1] != last or np.any(table < 0) or np.any(table > last) or np.any(np.diff(table) < 0))


def _segments_fill(probs, first_frame, first_seg, G, n_frames, seg_cap, prm, n_segs, seg_start, seg_end, mask, bad):
    if promise_broken(first_frame, n_frames) or promise_broken(first_seg, seg_cap):
        bad[:] = BAD_PROMISE
        return n_segs, seg_start, seg_end, mask, bad
    for g in range(G):
        f0, n, q0, cap = int(first_frame[g]), int(first_frame[g + 1] - first_frame[g]), int(first_seg[g]), int(first_seg[g + 1] - first_seg[g])
        if cap < (n + 1) // 2:
            bad[g] = BAD_CAPACITY
            continue
        st = stages(probs[f0:f0 + n], *prm)
        mask[f0:f0 + n] = mask_of(st[2], n)
        k = len(st[4])
        n_segs[g] = k
        seg_start[q0:q0 + k], seg_end[q0:q0 + k] = [s for s, _ in st[4]], [e for _, e in st[4]]
    return n_segs, seg_start, seg_end, mask, bad


def segments_launch(probs, first_frame, first_seg, on, off, open_len, close_len, min_run, max_gap, want_mask):
    """`vad_gpu.segments_launch` through the statement: the drivers of vad_gpu run on the CPU with this as their `launch`"""
    n_segs, seg_start, seg_end, mask, bad = segments_entry(np.asarray(probs), first_frame, first_seg, on, off, open_len, close_len, min_run,
                                                           max_gap)
    return n_segs, seg_start, seg_end, (mask if want_mask else None), bad


# ------------------------------------------------------------------ inputs

def built_probs(lengths, on=0.6, off=0.4, lead=0, tail=0) -> np.ndarray:
    """Alternating speech runs and gaps of the given lengths (speech first), `lead` / `tail` frames of silence around them: f32"""
    parts = [np.full(lead, 0.1)]
    for i, ln in enumerate(lengths):
        parts.append(np.full(ln, 0.9 if i % 2 == 0 else 0.1))
    parts.append(np.full(tail, 0.1))
    return np.concatenate(parts).astype(np.float32)


def prob_families(n: int, seed: int, on=0.6, off=0.4):
    """{name: f32 [n]}: the probability families of the GPU test for a recording of n frames"""
    rs = np.random.RandomState(seed)
    fam = {"uniform": rs.uniform(0, 1, n), "above": np.full(n, 0.9), "below": np.full(n, 0.1), "between": np.full(n, 0.5)}
    exact = rs.choice(np.array([on, off, 0.5, 0.9, 0.1], np.float32), n)
    fam["exact"] = exact
    nan = rs.uniform(0, 1, n)
    nan[rs.uniform(0, 1, n) < 0.3] = np.nan
    fam["nan"] = nan
    slow = np.repeat(rs.uniform(0, 1, n // 7 + 1), 7)[:n]                 # runs of 7 equal frames: long runs and gaps
    fam["slow"] = slow
    border = np.full(n, 0.1)
    border[: max(1, n // 3)] = 0.9
    border[n - max(1, n // 4):] = 0.9
    fam["borders"] = border
    lengths = []
    for L in (4, 5, 6, 8, 10, 25, 35):                                    # runs and gaps at L - 1, L, L + 1 for every length in use
        for d in (-1, 0, 1):
            lengths += [L + d, max(1, rs.randint(1, 40))]
            lengths += [max(1, rs.randint(1, 60)), L + d]
    built = built_probs(lengths, on, off, lead=rs.randint(0, 6))
    fam["built"] = np.resize(built, n) if n else built[:0]
    return {k: np.asarray(v, np.float32) for k, v in fam.items()}


def bursty_signal(seconds: float, seed: int, sr: int = 16000) -> np.ndarray:
    """Noise bursts of 0.2 to 1.5 s at -20 to -10 dBFS over a floor at -60 dBFS, with 30 ms ramps: f32"""
    rs = np.random.RandomState(seed)
    n = int(seconds * sr)
    env = np.full(n, 1e-3)
    at = int(rs.uniform(0.1, 0.6) * sr)
    while at < n:
        ln = int(rs.uniform(0.2, 1.5) * sr)
        env[at:at + ln] = 10 ** (rs.uniform(-20, -10) / 20)
        at += ln + int(rs.uniform(0.05, 0.9) * sr)
    k = int(0.03 * sr)
    env = np.convolve(env, np.ones(k) / k, mode="same")
    return (env * rs.standard_normal(n)).astype(np.float32)


def band_clean(y, win=480, hop=160, on=0.6, off=0.4, band=BAND) -> bool:
    """No float64 probability of the signal lies within `band` of a threshold: the condition under which f32 and f64 scorers decide alike"""
    p = energy_probs64(y, win, hop)
    return bool(np.all(np.abs(p - on) > band) and np.all(np.abs(p - off) > band))


# the signals of the GPU end-to-end tests: (seconds, seed); tests/test_vad_rules.py asserts every one band-clean
E2E_SIGNALS = ((3.0, 11), (7.3, 12), (12.0, 13), (0.5, 14), (20.0, 15))


def silent_signal(seconds: float, sr: int = 16000) -> np.ndarray:
    return (1e-4 * np.random.RandomState(5).standard_normal(int(seconds * sr))).astype(np.float32)
