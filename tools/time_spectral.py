"""Time the device spectral route on the GPU -> profiles/spectral_timing.json.

* ms per pass of sd_affinity_apply_f32 (device events around `reps` back-to-back passes after a warm-up; median of 5 such windows)
  and of sd_affinity_degree_f32, for N in {2000, 7609, 20000, 50000} and b in {16, 32}, with the bytes rate 4 N^2 / t stated against
  the 6.3 TB/s a copy achieves on the MI355X;
* the number of passes `cluster_gpu.estimate_num_speakers` and `cluster_gpu.spectral` take;
* both functions end to end at N = 7609 (a 1 h meeting at 2 s / 0.25 s windows) beside the two host functions of `cluster.py` in the
  same run on the same machine (host clock around work that ends in a device synchronise / a host result).

    python tools/time_spectral.py [--out profiles/spectral_timing.json] [--skip-host] [--sizes 2000,7609]
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

from speech_diarization_amd import cluster, cluster_gpu, ops  # noqa: E402

COPY_RATE = 6.3e12          # bytes / s, achievable HBM rate of a copy on the MI355X


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


def affinity(n, k, dev, seed=0):
    X, planted = R.planted_rows(n, k, 0.9, seed=seed, dtype=np.float32)
    return ops.cosine_affinity(torch.from_numpy(X).to(dev)), planted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_timing.json"))
    ap.add_argument("--sizes", default="2000,7609,20000,50000")
    ap.add_argument("--skip-host", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("time_spectral.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "copy_rate_TBps": COPY_RATE / 1e12, "passes": [], "routes": []}
    for n in [int(s) for s in a.sizes.split(",")]:
        K, planted = affinity(n, 8 if n < 20000 else 12, dev)
        deg = ops.affinity_degree(K, False)
        scale = torch.where(deg > 0, deg.rsqrt(), torch.ones_like(deg))
        reps = int(max(10, min(400, 2e11 / (4.0 * n * n))))          # about 0.1 .. 0.3 s of work per window
        ms, lo, hi = event_ms(lambda: ops.affinity_degree(K, False), reps)
        res["passes"].append({"entry": "sd_affinity_degree_f32", "N": n, "ms": ms, "ms_min": lo, "ms_max": hi, "reps": reps,
                              "TBps": 4.0 * n * n / (ms * 1e-3) / 1e12, "share_of_copy_rate": 4.0 * n * n / (ms * 1e-3) / COPY_RATE})
        for b in (16, 32):
            V = torch.randn((n, b), device=dev)
            ws = torch.empty((int(ops.N.load().sd_affinity_apply_workspace_bytes(n, b)),), dtype=torch.uint8, device=dev)
            ms, lo, hi = event_ms(lambda: ops.affinity_apply(K, scale, V, False, ws=ws), reps)
            rate = 4.0 * n * n / (ms * 1e-3)
            res["passes"].append({"entry": "sd_affinity_apply_f32", "N": n, "b": b, "ms": ms, "ms_min": lo, "ms_max": hi, "reps": reps,
                                  "TBps": rate / 1e12, "share_of_copy_rate": rate / COPY_RATE,
                                  "TFLOPs": 2.0 * n * n * b / (ms * 1e-3) / 1e12, "workspace_MB": ws.numel() / 1e6})
            print(json.dumps(res["passes"][-1]), flush=True)
        # the two functions on the device
        hi_spk = 12 if n < 20000 else 16
        for _ in range(2):                                            # the first round warms every shape up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k_dev, info_e = cluster_gpu.estimate_num_speakers(K, 2, hi_spk, assume_symmetric=True, return_info=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            lab_dev, info_s = cluster_gpu.spectral(K, k_dev, assume_symmetric=True, return_info=True)
            t2 = time.perf_counter()
        row = {"N": n, "speakers": int(k_dev), "device_estimate_s": t1 - t0, "device_spectral_s": t2 - t1,
               "estimate_passes": info_e["passes"], "spectral_passes": info_s["passes"], "block": 24,
               "planted_partition_recovered": bool(np.array_equal(cluster.relabel_by_first_appearance(lab_dev),
                                                                  cluster.relabel_by_first_appearance(planted)))}
        if n == 7609 and not a.skip_host:
            Kh = K.cpu().numpy()
            t0 = time.perf_counter()
            k_host = cluster.estimate_num_speakers(Kh, 2, hi_spk)
            t1 = time.perf_counter()
            lab_host = cluster.spectral(Kh, k_host)
            t2 = time.perf_counter()
            row.update(host_estimate_s=t1 - t0, host_spectral_s=t2 - t1, host_cpus=os.environ.get("OMP_NUM_THREADS", "unset"),
                       same_count=bool(k_host == k_dev),
                       same_partition=bool(np.array_equal(cluster.relabel_by_first_appearance(lab_host),
                                                          cluster.relabel_by_first_appearance(lab_dev))),
                       speedup=(t2 - t0) / (row["device_estimate_s"] + row["device_spectral_s"]))
        res["routes"].append(row)
        print(json.dumps(row), flush=True)
        del K
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
