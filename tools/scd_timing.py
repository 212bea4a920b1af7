"""Time the device speaker-change detection against pass 2 of the host route on the GPU host -> profiles/scd_timing.json.

Shapes: R recordings of S segments of W windows, (R, S, W) in {(256, 60, 25), (1024, 20, 25), (16, 400, 40), (1, 1, 18000)}: unit
"speaker" vectors of 192 floats that change with probability 0.08 per window, plus noise, drawn on the device.  The window embeddings
are RESIDENT on the device, where pass 1 (`encode_windows`) leaves them.
Routes, alternating in one process, three repetitions after a warm-up of both, host clock, minimum / median / maximum:
* device: `scd_gpu.split_rows_groups` from the rows on the device to the piece lists on the host: one upload of the tables, one
  launch, one copy back, the unpacking into Python lists (the part before the unpacking is also timed on its own line).
* host: pass 2 of `anti_stick_diarize.scd_split_segments(..., scd="host")`, restated here line for line because the function does not
  expose it: the rows come back to the host once (timed on its own line, and counted in the route), then for every segment
  `adjacent_cosine(embs, use_gpu=True)` (an upload, a launch and a synchronisation), numpy's mean and std, `scipy.signal.find_peaks`
  and the greedy loop, on this host's threads (torch's count is recorded).
The piece lists of the two routes are compared (equal segments are counted, not asserted: a timing input is not chosen for its
distance from the thresholds).  Also recorded: the kernel alone (device events), and the front of `diarize_many` (load, VAD, SCD,
segment embeddings; the seeded random-init encoder) on a folder of synthetic conversations with scd="host" and scd="device".

BAR, at the three folder shapes: the host's minimum over the device's maximum is at least 4.  The single segment of an hour has no bar.

    python tools/scd_timing.py [--out profiles/scd_timing.json] [--quick]
"""
import argparse
import gc
import json
import os
import sys
import time
import warnings

import numpy as np
import torch
from scipy.signal import find_peaks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from speech_diarization_amd import anti_stick_diarize as asd  # noqa: E402
from speech_diarization_amd import ops, scd_gpu, synth  # noqa: E402

RUNS = 3
SHAPES = [(256, 60, 25), (1024, 20, 25), (16, 400, 40), (1, 1, 18000)]
BAR = 4.0
HOP_MS, THR, MIN_SPEECH_MS, DIM = 200.0, 1.25, 1000.0, 192


def stats(ms):
    return {"min": float(min(ms)), "median": float(np.median(ms)), "max": float(max(ms))}


def make_rows(dev, n_segs, windows, seed):
    """-> f32 [n_segs * windows, DIM] on the device"""
    g = torch.Generator(device=dev).manual_seed(seed)
    n = n_segs * windows
    change = torch.rand((n,), generator=g, device=dev) < 0.08
    change[::windows] = True
    speaker = torch.cumsum(change.to(torch.int64), 0) - 1
    voices = torch.randn((int(speaker[-1]) + 1, DIM), generator=g, device=dev)
    return (voices[speaker] + 0.35 * torch.randn((n, DIM), generator=g, device=dev)).contiguous()


def host_pass2(embs_all, counts, starts, ends):
    """Pass 2 of `scd_split_segments` as it stands, on host rows -> one list of (start, end) per segment"""
    min_speech_s = MIN_SPEECH_MS / 1000.0
    out, off = [], 0
    for n, start, end in zip(counts, starts, ends):
        embs = embs_all[off: off + n]
        off += n
        dists = 1 - asd.adjacent_cosine(embs, True)
        z = (dists - dists.mean()) / dists.std() if np.std(dists) > 1e-6 else dists
        peaks, _ = find_peaks(z, height=THR)
        if peaks.size == 0:
            out.append([(start, end)])
            continue
        cuts = sorted(set(start + (peaks + 0.5) * HOP_MS / 1000.0))
        pieces, last = [], start
        for cut in cuts:
            if cut - last >= min_speech_s:
                pieces.append((last, cut))
                last = cut
        if end - last >= min_speech_s:
            pieces.append((last, end))
        out.append(pieces)
    return out


def event_ms(fn, windows=RUNS):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def case(dev, n_rec, segs_each, windows):
    n_segs = n_rec * segs_each
    rows = make_rows(dev, n_segs, windows, 1000 * n_rec + windows)
    counts = np.full(n_segs, windows, np.int64)
    first_row = np.concatenate([[0], np.cumsum(counts)])
    starts = [float(v) for v in 0.25 * np.arange(n_segs)]
    ends = [s + 1.0 + HOP_MS / 1000.0 * (windows - 1) for s in starts]

    def device():
        return [pieces for _, pieces in scd_gpu.split_rows_groups(rows, first_row, starts, ends, HOP_MS, THR, MIN_SPEECH_MS)]

    def host():
        return host_pass2(rows.cpu().numpy(), counts, starts, ends)
    got, want = device(), host()                                           # the warm-up of both
    first_piece = np.concatenate([[0], np.cumsum(scd_gpu.piece_capacity(counts))])
    ms = {"device": [], "host": [], "download": [], "launch": []}
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device()
        ms["device"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()                         # the part of the device route before the lists are made: upload, launch, copy back
        scd_gpu.split_launch(rows, first_row, np.asarray(starts), np.asarray(ends), first_piece, HOP_MS, THR, MIN_SPEECH_MS / 1000.0)
        ms["launch"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        host()
        ms["host"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        rows.cpu().numpy()
        ms["download"].append((time.perf_counter() - t0) * 1e3)
    row = {"recordings": n_rec, "segments_each": segs_each, "windows_each": windows, "segments": n_segs, "rows": int(rows.shape[0]),
           "device_ms": stats(ms["device"]), "device_upload_launch_copy_back_ms": stats(ms["launch"]), "host_ms": stats(ms["host"]), "download_of_the_rows_ms": stats(ms["download"]),
           "pieces": int(sum(len(w) for w in want)), "segments_split_on_the_host": int(sum(len(w) != 1 or w[0] != (s, e) for w, s, e in zip(want, starts, ends))),
           "segments_with_equal_pieces": int(sum(g == w for g, w in zip(got, want)))}
    row["host_min_over_device_max"] = row["host_ms"]["min"] / row["device_ms"]["max"]
    # the same device route with Python's cyclic collector off: what of its spread is collections set off by the lists it builds
    gc.collect()
    gc.disable()
    try:
        off = []
        for _ in range(RUNS):
            t0 = time.perf_counter()
            device()
            off.append((time.perf_counter() - t0) * 1e3)
    finally:
        gc.enable()
    row["device_with_the_collector_off_ms"] = stats(off)
    row["host_us_per_segment"] = 1e3 * row["host_ms"]["median"] / n_segs
    # the kernel alone
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)     # noqa: E731
    t_fr, t_fp, t_s, t_e = up(first_row, np.int32), up(first_piece, np.int32), up(starts, np.float64), up(ends, np.float64)
    ws = ops.Workspace(dev)
    row["kernel_ms"] = stats(event_ms(lambda: ops.scd_split_grouped(rows, t_fr, t_s, t_e, t_fp, int(first_piece[-1]), HOP_MS, THR,
                                                                     MIN_SPEECH_MS / 1000.0, ws=ws)))
    return row


def front_case(n_rec, seconds):
    """The front of `diarize_many` on `n_rec` synthetic conversations, both routes -> a row"""
    ys = [synth.synthetic_conversation(float(seconds), 2 + i % 2, seed=i).wav.astype(np.float32) for i in range(n_rec)]
    args = (16000, -18.0, 0.6, 0.4, 250, 100, 70.0, 80.0, 40.0, 1000.0, 200, 1.50, None, None, False)

    def front(route):
        return asd._diarize_fronts(ys, *args, route)
    pieces = {route: [[(s.start, s.end) for s in f[3]] if f else [] for f in front(route)] for route in ("device", "host")}      # the warm-up of both
    ms = {"device": [], "host": []}
    for _ in range(RUNS):
        for route in ("device", "host"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            front(route)
            torch.cuda.synchronize()
            ms[route].append((time.perf_counter() - t0) * 1e3)
    row = {"recordings": n_rec, "seconds_each": seconds, "front_device_ms": stats(ms["device"]), "front_host_ms": stats(ms["host"]),
           "segments_after_scd": int(sum(len(p) for p in pieces["host"])), "recordings_with_equal_pieces": int(sum(a == b for a, b in zip(pieces["device"], pieces["host"])))}
    row["host_min_over_device_max"] = row["front_host_ms"]["min"] / row["front_device_ms"]["max"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scd_timing.json"))
    ap.add_argument("--quick", action="store_true", help="16 recordings of 20 segments only, and a front of 4 conversations")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("scd_timing.py measures on the GPU; there is nothing to time without one")
    warnings.simplefilter("ignore", RuntimeWarning)      # the random-init encoder says that it is one
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "host_threads_torch": torch.get_num_threads(),
           "host_threads_env": os.environ.get("OMP_NUM_THREADS", "unset"),
           "parameters": f"hop {HOP_MS} ms, thr {THR}, min speech {MIN_SPEECH_MS} ms, rows of {DIM} floats",
           "bar_host_min_over_device_max_at_the_folder_shapes": BAR, "shapes": []}
    for n_rec, segs_each, windows in ([(16, 20, 25)] if a.quick else SHAPES):
        res["shapes"].append(case(dev, n_rec, segs_each, windows))
        print(json.dumps(res["shapes"][-1]), flush=True)
        torch.cuda.empty_cache()
    res["meets_the_bar"] = None if a.quick else bool(all(r["host_min_over_device_max"] >= BAR for r in res["shapes"][:3]))
    res["front_of_diarize_many"] = front_case(*((4, 20) if a.quick else (16, 60)))
    print(json.dumps(res["front_of_diarize_many"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
