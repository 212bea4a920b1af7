"""Time the device k-means against scikit-learn on the GPU host -> profiles/kmeans_timing.json.

Shapes: the folder shapes the project already uses, R recordings of m rows, (R, m, k) in {(256, 500, 4), (1024, 200, 4),
(16, 7609, 8)}, and single recordings of 7 609 rows (k = 8) and 50 000 rows (k = 12).  Each on two inputs:
* "spectral_like": planted blobs in k dimensions scaled by 1 / sqrt(m), the shape of a spectral embedding;
* "blobs": the overlapping blobs of the tests (8 columns, spread 1.0) scaled by 100.
Routes, alternating in one process, five repetitions after a warm-up of both, host clock, minimum / median / maximum:
* device: `kmeans_gpu.k_means_groups` from the rows on the device to the labels on the host (the draws on the host, the uploads of
  the tables, the two launches, one copy back);
* scikit-learn: `sklearn.cluster.k_means(..., n_init=10)` per recording on this host's threads (OMP_NUM_THREADS is recorded).
The labels of the two routes are compared (equal recordings are counted, not asserted: a timing input is not chosen for its margins).

BAR, folder shapes only: scikit-learn's minimum over the device's maximum is at least 2.  Single recordings have no bar: they run on
n_init workgroups.  Also recorded: `cluster_gpu.spectral` end to end at N = 7 609 with both `assign_labels`, and for the streamed case
(50 000 x 12: the rows do not fit in LDS) the bytes of rows one Lloyd iteration reads (two passes over n dim 8 bytes: the assignment
and the sums) over the kernel time per iteration of a single restart, seeding included in the time, next to a device copy's rate.

    python tools/kmeans_timing.py [--out profiles/kmeans_timing.json] [--quick]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import spectral_ref as R  # noqa: E402

from speech_diarization_amd import cluster_gpu, kmeans_gpu, ops  # noqa: E402

RUNS = 5
FOLDERS = [(256, 500, 4), (1024, 200, 4), (16, 7609, 8)]
SINGLES = [(1, 7609, 8), (1, 50000, 12)]
BAR = 2.0


def stats(ms):
    return {"min": float(min(ms)), "median": float(np.median(ms)), "max": float(max(ms))}


def spectral_like(m, k, seed):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((k, k))
    lab = rng.integers(0, k, m)
    return (C[lab] + 0.3 * rng.standard_normal((m, k))) / np.sqrt(m)


def blobs(m, k, seed):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((k, 8))
    lab = rng.integers(0, k, m)
    return 100.0 * (C[lab] + rng.standard_normal((m, 8)))


def host_route(parts, k):
    from sklearn.cluster import k_means
    return [k_means(x, k, random_state=np.random.RandomState(g), n_init=10)[1] for g, x in enumerate(parts)]


def case(dev, n_rec, m, k, kind, make):
    parts = [make(m, k, 1000 * n_rec + g) for g in range(n_rec)]
    Xd = torch.from_numpy(np.concatenate(parts)).to(dev)
    sizes = [m] * n_rec

    def device():
        return kmeans_gpu.k_means_groups(Xd, sizes, k, [np.random.RandomState(g) for g in range(n_rec)], return_info=True)

    def host():
        return host_route(parts, k)
    (got, info), want = device(), host()                                   # the warm-up of both
    ms = {"device": [], "sklearn": []}
    for _ in range(RUNS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        device()
        ms["device"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        host()
        ms["sklearn"].append((time.perf_counter() - t0) * 1e3)
    row = {"recordings": n_rec, "rows_each": m, "k": k, "dim": int(Xd.shape[1]), "input": kind, "device_ms": stats(ms["device"]),
           "sklearn_ms": stats(ms["sklearn"]), "fallback": len(info["fallback"]),
           "recordings_with_equal_labels": int(sum(np.array_equal(g, w) for g, w in zip(got, want))),
           "iterations_max": int(max(info["iterations"]))}
    row["sklearn_min_over_device_max"] = row["sklearn_ms"]["min"] / row["device_ms"]["max"]
    # the launches alone: device events around the two kernels
    first, u = np.zeros((n_rec, 10), np.int32), np.zeros((n_rec, 10, 31, 5))
    for g in range(n_rec):
        f, uu = kmeans_gpu.kmeans_draws(np.random.RandomState(g), m, k, 10)
        first[g], u[g, :, :uu.shape[1], :uu.shape[2]] = f, uu
    args = [torch.from_numpy(a).to(dev) for a in (np.arange(0, n_rec * m + 1, m, dtype=np.int32), np.full(n_rec, k, np.int32), first, u)]
    ws = ops.Workspace(dev)
    row["kernels_ms"] = stats(event_ms(lambda: ops.kmeans_grouped(Xd, *args, 10, 300, 1e-4, max_k=k, max_rows=m, ws=ws)))
    return row


def event_ms(fn, reps=3, windows=RUNS):
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


def streamed_rate(dev):
    """One restart of 50 000 x 12 (4.8 MB of rows: streamed from global memory): kernel time per Lloyd iteration, seeding included."""
    m, k = 50000, 12
    X = blobs(m, k, 7)[:, :8]
    X = np.concatenate([X, X[:, :4]], axis=1)
    Xd = torch.from_numpy(X).to(dev)
    f, uu = kmeans_gpu.kmeans_draws(np.random.RandomState(0), m, k, 1)
    u = np.zeros((1, 1, 31, 5))
    u[0, :, :uu.shape[1], :uu.shape[2]] = uu
    args = [torch.from_numpy(a).to(dev) for a in (np.array([0, m], np.int32), np.array([k], np.int32), f.reshape(1, 1), u)]
    out = ops.kmeans_grouped(Xd, *args, 1, 300, 1e-4, max_k=k, max_rows=m)
    iters = int(out[3].cpu()[0])
    ms = stats(event_ms(lambda: ops.kmeans_grouped(Xd, *args, 1, 300, 1e-4, max_k=k, max_rows=m)))
    big = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
    copy_ms = stats(event_ms(lambda: big.clone()))
    per_iter = 2 * m * 12 * 8
    return {"rows": m, "dim": 12, "k": k, "restarts": 1, "workgroups": 1, "iterations": iters, "kernels_ms": ms,
            "rows_bytes_read_per_lloyd_iteration": per_iter,
            "rows_bytes_per_iteration_over_kernel_time_per_iteration_GBps": per_iter * iters / (ms["median"] * 1e-3) / 1e9,
            "device_copy_256MiB_read_plus_write_GBps": 2 * (1 << 28) / (copy_ms["median"] * 1e-3) / 1e9,
            "note": "one workgroup on one of the device's compute units; the time includes the seeding (k - 1 steps of two passes each)"}


def spectral_end_to_end(dev, n=7609, k=8):
    X, _ = R.planted_rows(n, k, 1.2, seed=0, dtype=np.float32)
    Kd = ops.cosine_affinity(torch.from_numpy(X).to(dev))
    ms = {"sklearn": [], "device": []}
    labels = {}
    for name in ms:
        labels[name] = cluster_gpu.spectral(Kd, k, assume_symmetric=True, assign_labels=name)
    for _ in range(RUNS):
        for name in ms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            cluster_gpu.spectral(Kd, k, assume_symmetric=True, assign_labels=name)
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {"rows": n, "k": k, "assign_labels_sklearn_ms": stats(ms["sklearn"]), "assign_labels_device_ms": stats(ms["device"]),
            "equal_labels": bool(np.array_equal(labels["sklearn"], labels["device"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_timing.json"))
    ap.add_argument("--quick", action="store_true", help="the first folder shape and the first single recording only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("kmeans_timing.py measures on the GPU; there is nothing to time without one")
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    import sklearn
    res = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "n_init": 10, "host_threads": os.environ.get("OMP_NUM_THREADS", "unset"),
           "sklearn": sklearn.__version__, "bar_sklearn_min_over_device_max": BAR, "folders": [], "singles": []}
    for key, shapes in (("folders", FOLDERS[:1] if a.quick else FOLDERS), ("singles", SINGLES[:1] if a.quick else SINGLES)):
        for n_rec, m, k in shapes:
            for kind, make in (("spectral_like", spectral_like), ("blobs", blobs)):
                res[key].append(case(dev, n_rec, m, k, kind, make))
                print(json.dumps(res[key][-1]), flush=True)
                torch.cuda.empty_cache()
    res["folders_meet_the_bar"] = bool(all(r["sklearn_min_over_device_max"] >= BAR for r in res["folders"]))
    res["streamed"] = streamed_rate(dev)
    print(json.dumps(res["streamed"]), flush=True)
    res["spectral_end_to_end"] = spectral_end_to_end(dev)
    print(json.dumps(res["spectral_end_to_end"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
