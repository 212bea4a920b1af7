"""Time the grouped AHC route against one driver per recording on the GPU -> profiles/ahc_grouped_timing.json.

For folders of R planted recordings of m rows each, (R, m) in {(64, 500), (256, 500), (1024, 200), (16, 7609)} (8 planted speakers, cut
at cosine 0.3 as tools/time_ahc.py):
* `ahc_gpu.ahc_cosine_groups` over the folder and the loop of `ahc_gpu.ahc_cosine_rows` over its recordings (the baseline: that
  function is the parent's code), host clock around calls that end in a host result, the two alternating in one process: median, min
  and max of 5 runs each after a warm-up of both;
* rounds of both (the loop's sum and maximum), `gram_tiles`, the workspace bytes of both, the first grouped pass alone (device events);
* that both routes return the same labels.
The bar: at (256, 500) the loop's minimum over the grouped maximum is at least 4.  The per-round breakdown of the grouped driver at
that size (nearest, merge, read-back, compaction; a synchronise after each, so their sum exceeds the unsynchronised round) is recorded
beside it.

The embedding side, a record without a bar: the windows of a folder through `encode_windows` once per recording and once shared
(`diarize_audios`' layout: the signals concatenated with a window of zeros after each), as windows per second.

    python tools/ahc_grouped_timing.py [--out profiles/ahc_grouped_timing.json] [--cases 64x500,256x500] [--skip-embedding]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import spectral_ref as R  # noqa: E402

from speech_diarization_amd import _native, ahc_gpu, ops  # noqa: E402

COS_THR = 0.3
BAR_CASE, BAR = (256, 500), 4.0
RUNS = 5


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms))}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn, reps=20, windows=RUNS, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


class SteppedSums(ahc_gpu.DeviceSums):
    """DeviceSums that synchronises after every call and books the host time by step; what the driver does between a merge and the
    next nearest pass (read-back, compaction) is booked from the gaps."""

    def __init__(self, device):
        super().__init__(device)
        self.ms = {"nearest": 0.0, "merge": 0.0, "readback_and_compaction": 0.0}
        self.left = None

    def _timed(self, key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if self.left is not None and key == "nearest":
            self.ms["readback_and_compaction"] += (t0 - self.left) * 1e3
        out = fn()
        torch.cuda.synchronize()
        self.left = time.perf_counter()
        self.ms[key] += (self.left - t0) * 1e3
        return out

    def nearest_grouped(self, sums, inv_count, group, max_group):
        return self._timed("nearest", lambda: super(SteppedSums, self).nearest_grouped(sums, inv_count, group, max_group))

    def merge(self, sums, count, inv_count, nn, best, cos_thr):
        return self._timed("merge", lambda: super(SteppedSums, self).merge(sums, count, inv_count, nn, best, cos_thr))


def clustering_case(dev, n_rec, m):
    lib = _native.load()
    parts = [R.planted_rows(m, 8, 0.5, 1000 * n_rec + s, dtype=np.float32)[0] for s in range(n_rec)]
    Xd = torch.from_numpy(np.concatenate(parts)).to(dev)
    sizes = [m] * n_rec
    each = [Xd[i * m:(i + 1) * m] for i in range(n_rec)]
    op_g, op_l = ahc_gpu.DeviceSums(dev), ahc_gpu.DeviceSums(dev)

    def grouped():
        return ahc_gpu.ahc_cosine_groups(Xd, sizes, COS_THR, operator=op_g)

    def loop():
        return [ahc_gpu.ahc_cosine_rows(x, COS_THR, operator=op_l) for x in each]

    got, want = grouped(), loop()                                     # the warm-up of both, and the comparison
    t_g, t_l = [], []
    for _ in range(RUNS):                                             # alternating: other work shares the host
        t_g.append(wall_ms(grouped)[0])
        t_l.append(wall_ms(loop)[0])
    _, info = ahc_gpu.ahc_cosine_groups(Xd, sizes, COS_THR, operator=op_g, return_info=True)
    rounds = [ahc_gpu.ahc_cosine_rows(x, COS_THR, operator=op_l, return_info=True)[1]["rounds"] for x in each]
    Xn = op_g.normalise(Xd)
    ones = torch.ones(n_rec * m, device=dev)
    group = torch.arange(n_rec, dtype=torch.int32, device=dev).repeat_interleave(m)
    first = event_ms(lambda: op_g.nearest_grouped(Xn, ones, group, m))
    d = Xn.shape[1]
    row = {"recordings": n_rec, "rows_each": m, "rows": n_rec * m, "grouped_ms": stats(t_g), "loop_ms": stats(t_l),
           "loop_min_over_grouped_max": min(t_l) / max(t_g), "loop_median_over_grouped_median": float(np.median(t_l) / np.median(t_g)),
           "rounds_grouped": info["rounds"], "rounds_loop_sum": int(sum(rounds)), "rounds_loop_max": int(max(rounds)),
           "gram_tiles": info["gram_tiles"], "first_grouped_pass_ms": stats(first),
           "workspace_bytes_grouped": int(lib.sd_ahc_nearest_grouped_workspace_bytes(n_rec * m, d, m)),
           "workspace_bytes_loop": int(lib.sd_ahc_nearest_workspace_bytes(m, d)),
           "workspace_bytes_ungrouped_over_all_rows": int(lib.sd_ahc_nearest_workspace_bytes(n_rec * m, d)),
           "same_labels": bool(all(np.array_equal(g, w) for g, w in zip(got, want)))}
    if (n_rec, m) == BAR_CASE:
        step = SteppedSums(dev)
        ahc_gpu.ahc_cosine_groups(Xd, sizes, COS_THR, operator=step)
        row["grouped_round_breakdown_ms_synchronised"] = {k: v / max(1, info["rounds"] + 1) for k, v in step.ms.items()}
        row["bar"] = BAR
    return row


def embedding_case(dev, enc, n_rec, m, win=32000, hop=4000):
    """m windows at a hop of 0.25 s per recording; the signals are seeded noise made on the device, so neither route uploads."""
    length = (m - 1) * hop + win
    gen = torch.Generator(device=dev).manual_seed(n_rec * 100003 + m)
    signals = [0.1 * torch.randn(length, generator=gen, device=dev) for _ in range(n_rec)]
    starts = torch.arange(m, device=dev) * hop
    pad = torch.zeros(win, device=dev)
    shared = torch.cat([t for s in signals for t in (s, pad)])
    shared_starts = torch.cat([starts + i * (length + win) for i in range(n_rec)])

    def per_recording():
        return [enc.encode_windows(s, starts, win, to_host=False) for s in signals]

    def together():
        return enc.encode_windows(shared, shared_starts, win, to_host=False)

    a, b = torch.cat(per_recording()).double(), together().double()
    dist = float((1.0 - torch.nn.functional.cosine_similarity(a, b, dim=1)).max())
    t_p, t_s = [], []
    for _ in range(3):
        t_p.append(wall_ms(per_recording)[0])
        t_s.append(wall_ms(together)[0])
    n = n_rec * m
    return {"recordings": n_rec, "windows_each": m, "windows": n, "max_batch": enc.engine.max_batch,
            "per_recording_windows_per_s": stats([n / (t * 1e-3) for t in t_p]), "shared_windows_per_s": stats([n / (t * 1e-3) for t in t_s]),
            "shared_over_per_recording": float(np.median(t_p) / np.median(t_s)), "largest_rowwise_cosine_distance": dist}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ahc_grouped_timing.json"))
    ap.add_argument("--cases", default="64x500,256x500,1024x200,16x7609")
    ap.add_argument("--embedding-cases", default="64x500,160x200")
    ap.add_argument("--skip-embedding", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("ahc_grouped_timing.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "cos_thr": COS_THR, "runs": RUNS, "host_cpus": os.environ.get("OMP_NUM_THREADS", "unset"),
           "cases": [], "embedding": []}
    for n_rec, m in [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",") if c]:
        res["cases"].append(clustering_case(dev, n_rec, m))
        print(json.dumps(res["cases"][-1]), flush=True)
        torch.cuda.empty_cache()
    if not a.skip_embedding:
        from speech_diarization_amd import speech_encode, synth
        enc = speech_encode.HipEcapaEncoder(synth.make_ecapa_state_dict(1234), dev)
        for n_rec, m in [tuple(int(v) for v in c.split("x")) for c in a.embedding_cases.split(",") if c]:
            res["embedding"].append(embedding_case(dev, enc, n_rec, m))
            print(json.dumps(res["embedding"][-1]), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    bar = [r for r in res["cases"] if "bar" in r]
    if bar and bar[0]["loop_min_over_grouped_max"] < BAR:
        raise SystemExit(f"ahc_cosine_groups at {BAR_CASE} is {bar[0]['loop_min_over_grouped_max']:.2f} x the loop, the bar is {BAR} x")


if __name__ == "__main__":
    main()
