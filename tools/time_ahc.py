"""Time the device AHC route on the GPU -> profiles/ahc_timing.json.

For N in {2000, 7609, 20000, 50000} (planted rows, 8 or 12 speakers, cut at cosine 0.3):
* rounds, clusters, sum of n_active^2 over N^2;
* ms in the nearest passes (device events around every `nearest` call of one clustering) and ms in total (host clock around the call,
  which ends in a host result), each the median of 5 clusterings after a warm-up one;
* the first nearest pass (n_active = N) beside `sd_cosine_affinity_f32` at the same N in the same process (device events, median of 5
  windows of `reps` calls) and their ratio: the same N^2 D / 2 products, without the 4 N^2 bytes of output.
At N = 7609 (a 1 h meeting at 2 s / 0.25 s windows) the host route is timed in the same run: affinity download + `cluster.ahc_cosine`.

    python tools/time_ahc.py [--out profiles/ahc_timing.json] [--skip-host] [--sizes 2000,7609]
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

from speech_diarization_amd import ahc_gpu, cluster, ops  # noqa: E402

COS_THR = 0.3


def event_ms(fn, reps, windows=5, warmup=3):
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
    return float(np.median(out)), float(min(out)), float(max(out))


class TimedSums(ahc_gpu.DeviceSums):
    """DeviceSums with a pair of device events around every nearest pass."""

    def __init__(self, device):
        super().__init__(device)
        self.events = []

    def nearest(self, sums, inv_count):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = super().nearest(sums, inv_count)
        b.record()
        self.events.append((a, b))
        return out

    def nearest_ms(self):
        torch.cuda.synchronize()
        return float(sum(a.elapsed_time(b) for a, b in self.events))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ahc_timing.json"))
    ap.add_argument("--sizes", default="2000,7609,20000,50000")
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("time_ahc.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "cos_thr": COS_THR, "routes": []}
    for n in [int(s) for s in a.sizes.split(",")]:
        k = 8 if n < 20000 else 12
        X, planted = R.planted_rows(n, k, 0.5, 5, dtype=np.float32)
        Xd = torch.from_numpy(X).to(dev)
        # the first nearest pass beside the affinity kernel
        Xn = ops.l2norm_rows(Xd, sklearn_zero_guard=True)
        ones = torch.ones(n, device=dev)
        op = ahc_gpu.DeviceSums(dev)
        reps = int(max(5, min(200, 4e10 / (float(n) * n))))
        first_ms, first_lo, first_hi = event_ms(lambda: op.nearest(Xn, ones), reps)
        K = torch.empty((n, n), dtype=torch.float32, device=dev)
        aff_ms, aff_lo, aff_hi = event_ms(lambda: ops.cosine_affinity(Xd, out=K), reps)
        row = {"N": n, "planted_speakers": k, "first_nearest_ms": first_ms, "first_nearest_ms_min": first_lo, "first_nearest_ms_max": first_hi,
               "cosine_affinity_ms": aff_ms, "cosine_affinity_ms_min": aff_lo, "cosine_affinity_ms_max": aff_hi, "reps": reps,
               "first_nearest_over_affinity": first_ms / aff_ms, "first_nearest_TFLOPs": float(n) * n * X.shape[1] / (first_ms * 1e-3) / 1e12,
               "workspace_MB": op.ws.buf.numel() / 1e6}
        # the whole clustering
        total, near = [], []
        for it in range(6):                                           # the first one warms every shape up
            top = TimedSums(dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels, info = ahc_gpu.ahc_cosine_rows(Xd, COS_THR, operator=top, return_info=True)
            t1 = time.perf_counter()
            if it:
                total.append((t1 - t0) * 1e3)
                near.append(top.nearest_ms())
        row.update(rounds=info["rounds"], clusters=info["clusters"], gram_rows_over_N2=info["gram_rows"] / (float(n) * n),
                   last_best=info["last_best"], total_ms=float(np.median(total)), total_ms_min=float(min(total)), total_ms_max=float(max(total)),
                   nearest_ms=float(np.median(near)),
                   planted_partition_recovered=bool(np.array_equal(labels, cluster.relabel_by_first_appearance(planted))))
        if n == 7609 and not a.skip_host:
            host = []
            for _ in range(2):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                Kh = K.cpu().numpy()
                lab_host = cluster.ahc_cosine(Kh, COS_THR)
                host.append(time.perf_counter() - t0)
            row.update(host_route_s=float(min(host)), host_route_s_all=host, host_cpus=os.environ.get("OMP_NUM_THREADS", "unset"),
                       same_partition=bool(np.array_equal(cluster.relabel_by_first_appearance(lab_host), labels)),
                       speedup=float(min(host)) / (row["total_ms"] * 1e-3), speedup_bar=20.0)
        res["routes"].append(row)
        print(json.dumps(row), flush=True)
        del K, Xd, Xn
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    bar = [r for r in res["routes"] if "speedup" in r]
    if bar and bar[0]["speedup"] < bar[0]["speedup_bar"]:
        raise SystemExit(f"ahc_cosine_rows at N = 7609 is {bar[0]['speedup']:.1f} x the host route, the bar is 20 x")


if __name__ == "__main__":
    main()
