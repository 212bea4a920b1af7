"""The numpy statement of sd_scd_split_grouped_f32 (include/sd_hip_scd.h, rules 1-7), the margin of a segment, the float64 cosine
of adjacent rows, and the inputs the SCD tests share.

`split_from_cosines` is pass 2 of `anti_stick_diarize.scd_split_segments` restated in float64 from given f32 cosines.  The host does
the z-score in f32, so the two agree wherever no decision is close.  The MARGIN of a segment is the smallest distance of any of its
decisions from its threshold: |z - thr| over the candidate peaks, |std - 1e-6|, and |(cut - last) - min_speech_s| and
|(seg_end - last) - min_speech_s| over the decisions taken.  Its VALUE MARGIN is the smallest of the first two kinds alone: the
decisions about times are the same f64 operations on the host, in the statement and on the device, so they agree bit for bit however
close they are (at a hop of 200 ms and min_speech of 1 s two cuts five windows apart are 1 s apart up to rounding: one case in eight
has a time margin near 1e-16).  The tests compare every segment whose value margin is at least `MARGIN`: that is every segment whose
margin is, and more.

Imported as a helper (tests/helpers on sys.path)."""
import numpy as np

BAD_CAPACITY, BAD_PROMISE = 1, 2
LDS_ROWS = 2048
MARGIN = 1e-4
THRS = (1.0, 1.25, 1.5, 2.0)
FAMILIES = ("uniform", "eighths", "cauchy", "drops")


# ------------------------------------------------------------------ rules 3-7 of one segment

def peaks_of(d) -> list:
    """Rule 4 without the height: the maximal runs [l, r] of equal values with 1 <= l, r <= m - 2, d[l - 1] < d[l], d[r + 1] < d[r]
    -> their indices (l + r) // 2.  A NaN equals nothing and is below nothing."""
    d = np.asarray(d)
    m, out, l = len(d), [], 0
    while l < m:
        r = l
        while r + 1 < m and d[r + 1] == d[l]:
            r += 1
        if l >= 1 and r <= m - 2 and d[l - 1] < d[l] and d[r + 1] < d[r]:
            out.append((l + r) // 2)
        l = r + 1
    return out


def capacity(n: int) -> int:
    """The pieces a segment of n rows can emit: max(1, n // 2)"""
    return max(1, int(n) // 2)


def split_from_cosines(s32, seg_start: float, seg_end: float, hop_ms: float, thr: float, min_speech_s: float):
    """Rules 1-7 for a segment of len(s32) + 1 rows from its f32 cosines -> (kept peak indices, pieces [(start, end)], margin,
    value margin)."""
    s32 = np.asarray(s32, dtype=np.float32)
    seg_start, seg_end = float(seg_start), float(seg_end)
    if len(s32) + 1 < 3:
        return [], [(seg_start, seg_end)], np.inf, np.inf
    d = np.float32(1.0) - s32                                                   # f32, as on the host and on the device
    d64 = d.astype(np.float64)
    mean, std = d64.mean(), d64.std()
    margin = abs(std - 1e-6) if std == std else np.inf                          # a NaN: no decision is close
    z = (d64 - mean) / std if std > 1e-6 else d64
    kept = []
    for p in peaks_of(d):
        margin = min(margin, abs(z[p] - thr))
        if z[p] >= thr:
            kept.append(p)
    if not kept:
        return [], [(seg_start, seg_end)], margin, margin
    value_margin = margin
    cuts = []
    for p in kept:
        cut = seg_start + (p + 0.5) * hop_ms / 1000.0
        if not cuts or cut != cuts[-1]:
            cuts.append(cut)
    pieces, last = [], seg_start
    for cut in cuts:
        margin = min(margin, abs((cut - last) - min_speech_s))
        if cut - last >= min_speech_s:
            pieces.append((last, cut))
            last = cut
    margin = min(margin, abs((seg_end - last) - min_speech_s))
    if seg_end - last >= min_speech_s:
        pieces.append((last, seg_end))
    return kept, pieces, margin, value_margin


# ------------------------------------------------------------------ the entry

def split_entry(cos, first_row, seg_start, seg_end, hop_ms, thr, min_speech_s, first_piece, piece_fill=np.nan):
    """The outputs of the entry from the cosines in the layout of `sims` (cos[first_row[g] + i] = s_i; a segment's last slot is not
    looked at) -> dict(n_peaks, n_pieces, piece_start, piece_end, mask, bad, margin, value_margin); the slots of piece_start / piece_end that the
    entry leaves alone hold `piece_fill`."""
    cos = np.asarray(cos, dtype=np.float32)
    fr, fp = np.asarray(first_row, dtype=np.int64), np.asarray(first_piece, dtype=np.int64)
    G, n_rows = len(fr) - 1, len(cos)
    piece_cap = int(fp[-1]) if _promise(fp, None) else None
    out = dict(n_peaks=np.zeros(G, np.int32), n_pieces=np.zeros(G, np.int32), mask=np.zeros(n_rows, np.uint8), bad=np.zeros(G, np.int32),
               margin=np.full(G, np.inf), value_margin=np.full(G, np.inf))
    if not _promise(fr, n_rows) or piece_cap is None:
        raise ValueError("split_entry states the entry under the promise of its tables")
    out["piece_start"], out["piece_end"] = np.full(piece_cap, piece_fill, np.float64), np.full(piece_cap, piece_fill, np.float64)
    for g in range(G):
        r0, n, q0, cap = int(fr[g]), int(fr[g + 1] - fr[g]), int(fp[g]), int(fp[g + 1] - fp[g])
        if cap < capacity(n):
            out["bad"][g] = BAD_CAPACITY
            continue
        kept, pieces, out["margin"][g], out["value_margin"][g] = split_from_cosines(cos[r0:r0 + max(n - 1, 0)], seg_start[g], seg_end[g], hop_ms, thr, min_speech_s)
        assert len(pieces) <= capacity(n) and len(kept) <= max(n - 2, 0) // 2
        out["n_peaks"][g], out["n_pieces"][g] = len(kept), len(pieces)
        out["mask"][[r0 + p for p in kept]] = 1
        for k, (a, b) in enumerate(pieces):
            out["piece_start"][q0 + k], out["piece_end"][q0 + k] = a, b
    return out


def _promise(table, last) -> bool:
    return bool(table[0] == 0 and np.all(np.diff(table) >= 0) and (last is None or table[-1] == last))


def promise_holds(first_row, n_rows, first_piece, piece_cap) -> bool:
    return _promise(np.asarray(first_row, np.int64), n_rows) and _promise(np.asarray(first_piece, np.int64), piece_cap)


def sims_layout(cos_list) -> np.ndarray:
    """The cosines of the segments (one f32 vector of n - 1 values per segment of n >= 1 rows; an empty segment has none and is given
    as None) in the layout of `sims`: the last slot of every segment NaN."""
    parts = []
    for c in cos_list:
        if c is not None:
            parts += [np.asarray(c, np.float32), np.array([np.nan], np.float32)]
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def cosines64(rows, eps: float = 1e-8) -> np.ndarray:
    """<e_i, e_{i+1}> / (|e_i| |e_{i+1}| + eps) of adjacent rows in float64 [REF anti_stick_diarize.py:102-104]"""
    e = np.asarray(rows, dtype=np.float64)
    a, b = e[:-1], e[1:]
    return np.einsum("id,id->i", a, b) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) + eps)


def numpy_launch(rows, first_row, seg_start, seg_end, first_piece, hop_ms, thr, min_speech_s):
    """The launch of `scd_gpu.split_rows_groups` on the host (`launch=`): float64 cosines of the rows rounded to f32, then the
    statement -> (n_peaks, n_pieces, piece_start, piece_end, bad) as numpy."""
    rows = np.asarray(rows, dtype=np.float32)
    fr = np.asarray(first_row, dtype=np.int64)
    cos = sims_layout([cosines64(rows[a:b]).astype(np.float32) if b > a else None for a, b in zip(fr[:-1], fr[1:])])
    out = split_entry(cos, fr, seg_start, seg_end, hop_ms, thr, min_speech_s, first_piece)
    return out["n_peaks"], out["n_pieces"], out["piece_start"], out["piece_end"], out["bad"]


# ------------------------------------------------------------------ inputs

def cosine_family(name: str, m: int, rs) -> np.ndarray:
    """m cosines of one of the four families, f32"""
    if name == "uniform":
        s = rs.uniform(0.2, 1.0, m)
    elif name == "eighths":
        s = np.round(rs.uniform(0.2, 1.0, m) * 8) / 8
    elif name == "cauchy":
        s = 1.0 - 0.01 * np.abs(rs.standard_cauchy(m))
    elif name == "drops":
        s = np.where(rs.uniform(0, 1, m) < 0.15, rs.uniform(0.1, 0.6, m), rs.uniform(0.9, 1.0, m))
    else:
        raise ValueError(name)
    return s.astype(np.float32)


def rows_with_cosines(s, dim: int, rs, scale=None) -> np.ndarray:
    """len(s) + 1 rows of `dim` floats whose adjacent cosines are close to s (clipped to [-1, 1]): each row is the one before it turned
    by acos(s_i) towards a random direction, times a random length"""
    s = np.clip(np.asarray(s, dtype=np.float64), -1.0, 1.0)
    u = rs.standard_normal(dim)
    u /= np.linalg.norm(u)
    out = [u]
    for c in s:
        w = rs.standard_normal(dim)
        w -= w.dot(u) * u
        w /= np.linalg.norm(w)
        u = c * u + np.sqrt(max(0.0, 1.0 - c * c)) * w
        u /= np.linalg.norm(u)
        out.append(u)
    e = np.stack(out)
    lengths = rs.uniform(0.5, 2.0, (len(e), 1)) if scale is None else scale
    return (e * lengths).astype(np.float32)


def codebook_rows(word: str, dim: int, seed: int = 0) -> np.ndarray:
    """One row per letter of `word` from a codebook of random vectors: equal letters are equal rows, so every pair (A, A) has one
    cosine, and the cosine of (A, B) has the bits of (B, A): the products and the two norms commute."""
    rs = np.random.RandomState(seed)
    book = {ch: rs.standard_normal(dim).astype(np.float32) for ch in sorted(set(word))}
    return np.stack([book[ch] for ch in word])


def random_launch(seed: int = 11, n_segs: int = 200, dim: int = 16):
    """The random launch of the GPU tests: `n_segs` segments of 3-40 rows of `dim` floats, the four families in turn driven through
    `rows_with_cosines` -> (rows per segment, first_row, seg_start, seg_end)"""
    rs = np.random.RandomState(seed)
    rows = [rows_with_cosines(cosine_family(FAMILIES[g % 4], rs.randint(3, 41) - 1, rs), dim, rs) for g in range(n_segs)]
    counts = np.array([len(r) for r in rows])
    starts = 0.25 * rs.randint(0, 4000, n_segs)
    return rows, np.concatenate([[0], np.cumsum(counts)]), starts, starts + 1.0 + 0.2 * (counts - 1) + 0.07


def long_segment(seed: int = 12, dim: int = 8):
    """One segment of LDS_ROWS + 1 rows: the smallest whose distances, cuts and chain live in the workspace"""
    rs = np.random.RandomState(seed)
    rows = [rows_with_cosines(cosine_family("drops", LDS_ROWS, rs), dim, rs)]
    return rows, np.array([0, LDS_ROWS + 1]), np.array([12.5]), np.array([12.5 + 1.0 + 0.2 * LDS_ROWS])
