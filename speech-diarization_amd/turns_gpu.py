"""Device route for the speaker turns: the window labels of all recordings of a folder to their relabelled labels and turns, in one launch.

`cluster.relabel_by_first_appearance` is a Python loop over every window, and `diarization_baseline.labels_to_turns` builds, per speech
region, a frames x windows distance matrix, takes its argmin and run-length encodes it in Python.  Here the same rules are one upload,
one launch and one download for every recording (include/sd_hip_turns.h, `sd_turns_grouped`): inside a region the window a frame belongs
to never decreases, so every window finds the first frame it owns by a binary search on the host's own f64 comparison, and the runs come
out of two block scans.  The kernel returns integer runs (region, first frame, end frame, label); the times are made here with the
host's own expression, so the turns are the host's, value for value.

The launch is injectable (`launch=`), as in scd_gpu: the CPU tests run the packing and the unpacking through the numpy statement of the
entry.  There is no implicit CPU route: the product launch refuses to run without a GPU.
"""
from __future__ import annotations

import numpy as np
import torch

from .device_rows import DeviceRoute

BAD_LABEL, BAD_PROMISE = 1, 2


class DeviceTurns(DeviceRoute):
    route, takes = "turns", "the labels"


_routes: dict = {}


def _route(device) -> DeviceTurns:
    """The route of a device, its workspace kept between calls."""
    dev = DeviceTurns.guard(device)
    if not torch.cuda.is_available():
        raise RuntimeError("the device turns route runs on the HIP path (a visible GPU); there is no CPU fallback")
    dev = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
    if dev not in _routes:
        _routes[dev] = DeviceTurns(dev)
    return _routes[dev]


def turns_launch(first_window, first_region, region_first_window, centre, region_start, n_frames, frame_s, labels, device="cuda"):
    """The product launch: ONE upload of the seven tables, `ops.turns_grouped`, and ONE synchronisation, the copy of its results ->
    numpy (new_labels, n_runs, run_region, run_first, run_end, run_label, bad)."""
    from . import ops
    route = _route(device)
    G, R, W = len(first_window) - 1, len(region_first_window) - 1, len(labels)
    host = np.concatenate([np.asarray(centre, np.float64).view(np.uint8), np.asarray(region_start, np.float64).view(np.uint8)] +
                          [np.asarray(t, np.int32).view(np.uint8) for t in (first_window, first_region, region_first_window, n_frames, labels)])
    tables = torch.from_numpy(host).to(route.device)
    at, parts = 0, []
    for count, dt, size in ((W, torch.float64, 8), (R, torch.float64, 8), (G + 1, torch.int32, 4), (G + 1, torch.int32, 4),
                            (R + 1, torch.int32, 4), (R, torch.int32, 4), (W, torch.int32, 4)):
        parts.append(tables[at:at + count * size].view(dt))
        at += count * size
    t_centre, t_start, t_fw, t_fr, t_rfw, t_frames, t_labels = parts
    new_labels, n_runs, run_region, run_first, run_end, run_label, bad = ops.turns_grouped(t_fw, t_fr, t_rfw, t_centre, t_start, t_frames,
                                                                                          float(frame_s), t_labels, ws=route.ws)
    ints = torch.cat([new_labels, run_region, run_first, run_end, run_label, n_runs, bad]).cpu().numpy()      # one copy
    return ints[:W], ints[5 * W:5 * W + G], ints[W:2 * W], ints[2 * W:3 * W], ints[3 * W:4 * W], ints[4 * W:5 * W], ints[5 * W + G:]


def turn_times(speech, run_region, run_first, run_end, run_label, frame_s: float) -> list:
    """The runs of ONE recording as `labels_to_turns` writes its turns: round(s + a * frame_s, 3) and round(min(e, s + b * frame_s), 3)
    with `a` and `b` numpy integers, so that the sums are numpy float64 and `round` is numpy's rounding, as on the host.  Vectorised:
    numpy's rounding of the whole vectors is its rounding of each numpy float64; where `min` returns the region's own end `e` (a run
    that reaches it), `round` is applied to that object as on the host, where it may be a Python float with Python's rounding.
    `turn_times_scalar` is the host's expression run by run; tests/test_turns_rules.py holds the two equal."""
    r = np.asarray(run_region, dtype=np.int64)
    if r.size == 0:
        return []
    s = np.array([x for x, _ in speech], dtype=np.float64)[r]
    e = np.array([x for _, x in speech], dtype=np.float64)[r]
    first = np.round(s + np.asarray(run_first, dtype=np.int64) * frame_s, 3)
    stop = s + np.asarray(run_end, dtype=np.int64) * frame_s
    ends = list(np.round(stop, 3))
    for k in np.flatnonzero(~(stop < e)).tolist():       # min(e, x) is x only when x < e
        ends[k] = round(speech[r[k]][1], 3)
    return list(zip(first, ends, np.asarray(run_label).tolist()))


def turn_times_scalar(speech, run_region, run_first, run_end, run_label, frame_s: float) -> list:
    """`turn_times` with the host's expression itself, one run at a time."""
    turns = []
    for r, a, b, k in zip(np.asarray(run_region).tolist(), np.asarray(run_first, dtype=np.int64), np.asarray(run_end, dtype=np.int64),
                          np.asarray(run_label).tolist()):
        s, e = speech[r]
        turns.append((round(s + a * frame_s, 3), round(min(e, s + b * frame_s), 3), int(k)))
    return turns


def labels_to_turns_groups(speech_list, centres_list, regions_list, labels_list, frame_s: float = 0.01, launch=None):
    """`cluster.relabel_by_first_appearance` then `diarization_baseline.labels_to_turns` for every recording in one launch and one
    download: recording g has the speech regions speech_list[g] ([(start_s, end_s)]), the window centres centres_list[g] (seconds) with
    their region indices regions_list[g] (both as `speech_windows` returns them; None or empty for a recording without windows) and
    the window labels labels_list[g] -> one (relabelled labels, [(start_s, end_s, label)]) per recording, equal to the host's.
    ValueError where the regions of a recording decrease or the centres do not increase strictly inside a region: the windows of a
    region must be contiguous and ordered (the host route, `labels_to_turns`, takes such input)."""
    G = len(speech_list)
    if not (len(centres_list) == len(regions_list) == len(labels_list) == G):
        raise ValueError(f"one speech list, centre array, region array and label array per recording, got {G}, {len(centres_list)}, "
                         f"{len(regions_list)} and {len(labels_list)}")
    frame_s = float(frame_s)
    if not (frame_s > 0 and np.isfinite(frame_s)):
        raise ValueError(f"frame_s must be positive and finite, got {frame_s}")
    centres, labels, rfw, starts, frames, sizes, region_counts = [], [], [], [], [], [], []
    offset = 0
    for g, (speech, c, reg, lab) in enumerate(zip(speech_list, centres_list, regions_list, labels_list)):
        c = np.zeros(0, np.float64) if c is None else np.asarray(c, dtype=np.float64)
        reg = np.zeros(0, np.int64) if reg is None else np.asarray(reg, dtype=np.int64)
        lab = np.zeros(0, np.int64) if lab is None else np.asarray(lab)
        if not (c.ndim == reg.ndim == lab.ndim == 1 and len(c) == len(reg) == len(lab)):
            raise ValueError(f"recording {g}: {c.shape} centres, {reg.shape} regions and {lab.shape} labels")
        nr = len(speech)
        if len(reg) and (reg.min() < 0 or reg.max() >= nr or np.any(np.diff(reg) < 0)):
            raise ValueError(f"recording {g}: the region indices must lie in [0, {nr}) and must not decrease "
                             "(labels_to_turns, the host route, takes such windows)")
        if len(c) > 1 and not np.all((np.diff(c) > 0) | (np.diff(reg) > 0)):
            raise ValueError(f"recording {g}: the window centres must increase strictly inside a region "
                             "(labels_to_turns, the host route, takes such windows)")
        if len(lab) and (lab.max() >= 2 ** 31 or lab.min() < -2 ** 31):
            raise ValueError(f"recording {g}: labels outside int32")
        centres.append(c), labels.append(lab.astype(np.int64))
        rfw.append(offset + np.searchsorted(reg, np.arange(nr)))           # the first window of every region (a region may have none)
        starts.append(np.array([s for s, _ in speech], dtype=np.float64))
        frames.append(np.array([max(1, int(round((e - s) / frame_s))) for s, e in speech], dtype=np.int64))   # as labels_to_turns counts
        sizes.append(len(c)), region_counts.append(nr)
        offset += len(c)
    if offset >= 2 ** 31 or sum(region_counts) >= 2 ** 31 or any(f.size and f.max() >= 2 ** 31 for f in frames):
        raise ValueError("the windows, regions and frames of a launch are counted in int32")
    first_window = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    first_region = np.concatenate([[0], np.cumsum(region_counts)]).astype(np.int64)
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)      # noqa: E731
    region_first_window = np.concatenate([cat(rfw, np.int64), [offset]]).astype(np.int64)
    if launch is None:
        launch = turns_launch                            # looked up at the call: the product launch, which refuses to run without a GPU
    if G == 0:
        return []
    new_labels, n_runs, run_region, run_first, run_end, run_label, bad = launch(
        first_window, first_region, region_first_window, cat(centres, np.float64), cat(starts, np.float64), cat(frames, np.int64), frame_s,
        cat(labels, np.int64))
    bad = np.asarray(bad)
    if np.any(bad):
        raise RuntimeError(f"sd_turns_grouped refused recording(s) {np.flatnonzero(bad).tolist()}: flags {bad[bad != 0].tolist()}")
    out = []
    for g, speech in enumerate(speech_list):
        a, b = int(first_window[g]), int(first_window[g + 1])
        k = slice(a, a + int(n_runs[g]))
        out.append((np.asarray(new_labels[a:b]).astype(int), turn_times(speech, run_region[k], run_first[k], run_end[k], run_label[k], frame_s)))
    return out
