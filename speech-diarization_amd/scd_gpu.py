"""Device route for speaker-change detection: the window embeddings of all segments of a folder to their split pieces, in one launch.

Pass 2 of `anti_stick_diarize.scd_split_segments` takes the window embeddings of ONE segment at a time: it uploads them, launches the
adjacent cosine, synchronises to download a handful of floats, and does the z-score, `scipy.signal.find_peaks` and the greedy cut
filter in Python.  Here the same rules are one launch and one download for every segment of every recording
(include/sd_hip_scd.h, `sd_scd_split_grouped_f32`): the embeddings stay where `encode_windows(..., to_host=False)` left them.

The cosines are those of `ops.adjacent_cosine`, bit for bit; the z-score is f64 where the host's is f32, so the pieces are the host's
wherever no peak lies within the f32 rounding of the threshold; the times are the host's f64 values.

The launch is injectable (`launch=`), as in vad_gpu: the CPU tests run the packing and the unpacking through the numpy statement of the
entry.  There is no implicit CPU route: the product launch refuses rows that are not a GPU tensor.
"""
from __future__ import annotations

import numpy as np
import torch

from .device_rows import DeviceRoute

BAD_CAPACITY, BAD_PROMISE = 1, 2


class DeviceScd(DeviceRoute):
    route, takes = "SCD", "the window embeddings"


def piece_capacity(n_rows) -> np.ndarray:
    """The pieces a segment of n rows can emit, max(1, n // 2): a segment's share of piece_start / piece_end."""
    return np.maximum(np.asarray(n_rows, dtype=np.int64) // 2, 1)


def split_launch(rows, first_row, seg_start, seg_end, first_piece, hop_ms, thr, min_speech_s):
    """The product launch: ONE upload of the four tables, `ops.scd_split_grouped` on the device of the rows, and ONE synchronisation,
    the copy of its results -> numpy (n_peaks, n_pieces, piece_start, piece_end, bad)."""
    from . import ops
    dev, G, cap = DeviceScd.guard(rows), len(seg_start), int(first_piece[-1])
    host = np.concatenate([np.asarray(seg_start, np.float64).view(np.uint8), np.asarray(seg_end, np.float64).view(np.uint8),
                           np.asarray(first_row, np.int32).view(np.uint8), np.asarray(first_piece, np.int32).view(np.uint8)])
    tables = torch.from_numpy(host).to(dev)
    t_start, t_end = tables[:8 * G].view(torch.float64), tables[8 * G:16 * G].view(torch.float64)
    t_row, t_piece = tables[16 * G:16 * G + 4 * (G + 1)].view(torch.int32), tables[16 * G + 4 * (G + 1):].view(torch.int32)
    n_peaks, n_pieces, piece_start, piece_end, _, _, bad = ops.scd_split_grouped(rows, t_row, t_start, t_end, t_piece, cap, hop_ms, thr,
                                                                                min_speech_s)
    packed = torch.cat([t.view(torch.uint8) for t in (piece_start, piece_end, n_peaks, n_pieces, bad)]).cpu().numpy()   # one copy
    times, ints = packed[:16 * cap].view(np.float64), packed[16 * cap:].view(np.int32)
    return ints[:G], ints[G:2 * G], times[:cap], times[cap:], ints[2 * G:]


def split_rows_groups(rows_dev, first_row, seg_start, seg_end, hop_ms: float, thr: float, min_speech_ms: float, launch=None):
    """Pass 2 of `scd_split_segments` for every segment in one launch and one download: segment g owns the window embeddings
    rows_dev[first_row[g] : first_row[g + 1]] (f32 [n_rows, dim] on the device; first_row: G + 1 non-decreasing integers from 0 to
    n_rows) and lies between seg_start[g] and seg_end[g] seconds -> one (n_peaks, [(start_s, end_s), ...]) per segment.  A segment of
    fewer than 3 rows, or without a peak, has n_peaks == 0 and its own (seg_start, seg_end) as the one piece."""
    first_row = np.asarray(first_row, dtype=np.int64)
    seg_start, seg_end = np.asarray(seg_start, dtype=np.float64), np.asarray(seg_end, dtype=np.float64)
    counts = np.diff(first_row)
    if first_row.ndim != 1 or first_row.size < 2 or first_row[0] != 0 or np.any(counts < 0) or first_row[-1] != int(rows_dev.shape[0]):
        raise ValueError("first_row must run from 0 to the number of rows without decreasing, one entry more than segments")
    if seg_start.shape != counts.shape or seg_end.shape != counts.shape:
        raise ValueError(f"seg_start and seg_end must hold one time per segment, got {seg_start.shape} and {seg_end.shape} for {counts.size}")
    if not hop_ms > 0:
        raise ValueError(f"hop_ms must be positive, got {hop_ms}")
    first_piece = np.concatenate([[0], np.cumsum(piece_capacity(counts))]).astype(np.int64)
    if launch is None:
        launch = split_launch                            # looked up at the call: the product launch, which refuses host rows
    n_peaks, n_pieces, piece_start, piece_end, bad = launch(rows_dev, first_row, seg_start, seg_end, first_piece, float(hop_ms), float(thr),
                                                            float(min_speech_ms) / 1000.0)
    if np.any(bad):
        raise RuntimeError(f"sd_scd_split_grouped_f32 refused segment(s) {np.flatnonzero(bad).tolist()}: flags {bad[bad != 0].tolist()}")
    ps, pe = np.asarray(piece_start).tolist(), np.asarray(piece_end).tolist()      # Python floats once, not one conversion per piece
    return [(k, list(zip(ps[q:q + c], pe[q:q + c]))) for k, q, c in zip(np.asarray(n_peaks).tolist(), first_piece[:-1].tolist(),
                                                                        np.asarray(n_pieces).tolist())]
