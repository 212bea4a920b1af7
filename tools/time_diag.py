"""Time the f64 whitening / centroid entries and the device route of `diar_diag.resegment` on the GPU -> profiles/diag_timing.json.

For N in {300, 3000, 20000, 50000} planted low-rank rows (d = 192, tests/helpers/diag_cases.planted_lowrank, 8 speakers):

* the three entries of include/sd_hip_diag.h (`ops.whiten_stats`, `ops.whiten_apply`, `ops.label_centroids` with k = 8): device events,
  median of 5 windows of `reps` calls after 3 warm-up calls, and the f64 FLOP/s of the two matrix-core entries computed from the shape
  (stats: N d (d + 1) multiply-adds on the upper triangle; apply: N d^2);
* `resegment(device="cuda")` with the defaults (whitening, HDBSCAN, AS-norm, Viterbi) on rows that are already on the device: wall
  time ending in a synchronise, median of 3 after a warm-up run; beside it, up to --host-max rows, `resegment(device=None)` once on
  this machine's CPUs (the core count is recorded; above --host-max the host route's N x N float64 matrices are not attempted and the
  entry says "not measured");
* the bytes that cross the bus in each route, computed from the shapes and the measured HDBSCAN rounds.

    python tools/time_diag.py [--out profiles/diag_timing.json] [--host-max 3000] [--sizes 300,3000,20000,50000]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import diag_cases as DC  # noqa: E402

from speech_diarization_amd import diag_gpu, hdbscan_gpu, ops  # noqa: E402
from speech_diarization_amd import diar_diag as dd  # noqa: E402

D, K = 192, 8


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
    return {"median_ms": float(np.median(out)), "min_ms": float(min(out)), "max_ms": float(max(out)), "reps": reps}


def entries(X, labels):
    n = X.shape[0]
    reps = int(max(10, min(200, 2e6 / n)))
    ws = torch.empty((int(ops.N.load().sd_whiten_stats_workspace_bytes(n, D)),), dtype=torch.uint8, device=X.device)
    mean, gram = ops.whiten_stats(X, ws=ws)
    W = torch.from_numpy(diag_gpu.whitening_matrix(gram.cpu().numpy(), n)).to(X.device)
    row = {"whiten_stats": event_ms(lambda: ops.whiten_stats(X, ws=ws), reps), "whiten_apply": event_ms(lambda: ops.whiten_apply(X, mean, W), reps),
           "label_centroids_k8": event_ms(lambda: ops.label_centroids(X, labels, K), reps), "stats_workspace_MB": ws.numel() / 1e6}
    row["whiten_stats_f64_GFLOPs"] = 2.0 * n * D * (D + 1) / 2 / (row["whiten_stats"]["median_ms"] * 1e-3) / 1e9
    row["whiten_apply_f64_GFLOPs"] = 2.0 * n * D * D / (row["whiten_apply"]["median_ms"] * 1e-3) / 1e9
    return row


def bus_bytes(n, k, rounds):
    """What each route moves between host and device, from the shapes (rows already on the device after the encoder)."""
    pairs = min(2000, 4 * n)
    device = {"down_gram_and_mean": D * D * 8, "up_whitening_matrix": D * D * 8, "down_hdbscan_rounds": rounds * n * 8, "up_components": rounds * n * 4,
              "up_centre_index": n * 4, "down_centres": k * D * 4, "down_path": n * 4, "down_adjacent": (n - 1) * 4, "up_pair_sample": 2 * pairs * 8,
              "down_pair_cosines": pairs * 4}
    device["total"] = int(sum(device.values()))
    return {"device_route": device, "host_route": {"down_embeddings": n * D * 4, "total": n * D * 4}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_timing.json"))
    ap.add_argument("--host-max", type=int, default=3000)
    ap.add_argument("--sizes", default="300,3000,20000,50000")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("time_diag.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "host_cpus": os.environ.get("OMP_NUM_THREADS", "unset"), "d": D, "planted_speakers": K, "sizes": []}
    for n in (int(s) for s in a.sizes.split(",")):
        Xh, planted = DC.planted_lowrank(n, K, 12, 0.4, 4)
        X = torch.from_numpy(Xh).to(dev)
        row = {"N": n, "entries": entries(X, torch.from_numpy(planted.astype(np.int32)).to(dev))}
        segs = [[i * 1.0, i * 1.0 + 0.8] for i in range(n)]
        got = dd.resegment(X, segs, device=dev)                        # warm-up: every shape, the workspace, scikit-learn's imports
        torch.cuda.synchronize()
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = dd.resegment(X, segs, device=dev)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
        _, info = hdbscan_gpu.hdbscan_rows(diag_gpu.whiten_l2_rows(X), 6, 3, False, "cosine", return_info=True)
        k = len(got["centers"])
        row["resegment_device"] = {"median_s": float(np.median(wall)), "min_s": float(min(wall)), "max_s": float(max(wall)), "clusters": k,
                                   "noise_rows": int((got["labels"] < 0).sum()), "hdbscan_rounds": info["rounds"],
                                   "viterbi": "device" if k <= 64 else "host"}
        if n <= a.host_max:
            t0 = time.perf_counter()
            host = dd.resegment(Xh, segs)
            row["resegment_host"] = {"seconds": time.perf_counter() - t0, "clusters": len(host["centers"]),
                                     "same_final_partition": bool(len(set(zip(host["final_labels"].tolist(), got["final_labels"].tolist())))
                                                                  == len(set(host["final_labels"].tolist())) == len(set(got["final_labels"].tolist())))}
            row["speedup"] = row["resegment_host"]["seconds"] / row["resegment_device"]["median_s"]
        else:
            row["resegment_host"] = f"not measured: above --host-max {a.host_max} rows (N x N float64 matrices: {n * n * 8 / 1e9:.1f} GB each)"
        row["bus_bytes"] = bus_bytes(n, k, info["rounds"])
        row["hdbscan_rounds_bound"] = int(math.ceil(math.log2(n)))
        res["sizes"].append(row)
        print(json.dumps(row), flush=True)
        del X
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:                                    # after every size: a later size that fails keeps the earlier ones
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
