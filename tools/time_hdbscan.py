"""Time the device HDBSCAN route on the GPU -> profiles/hdbscan_timing.json.

* Kernel cost at N = 7609 and N = 50000 (d = 192, planted unit rows): one `sd_hdb_outgoing_f32` pass with all-singleton components
  beside one `sd_ahc_nearest_f32` pass at the same shape in the same process (both run the one tile and argmax of
  csrc/sd_gram_tile.h), their ratio against the bar of 1.25, and the core pass (`sd_hdb_core_f32`, k = 1 and 2: a full-Gram pass)
  beside them.  Device events, median of 5 windows of `reps` calls after 3 warm-up calls.
* End to end at N = 7609 (a 1 h meeting at 2 s / 0.25 s windows; 8 planted speakers): `hdbscan_rows` at (2, None, True) "euclidean"
  and at (6, 3, False) "cosine", each the median of 5 clusterings after a warm-up one, with the rounds, the ms inside the kernels
  (device events around every operator call) and the ms of the host tree step (scikit-learn's `_process_mst` + `tree_to_labels`);
  beside them, once each on the same machine's CPUs: the host clusterer at the same settings (scikit-learn's HDBSCAN on the rows;
  `cluster.hdbscan_precomputed` on the downloaded affinity) and the two-stage glue with either factory.  The device route must be
  faster (the tool exits non-zero otherwise); the ratio is recorded, no number is fixed for it.
* At N = 50000, 12 planted speakers: wall time and rounds of one clustering at (15, 5, True); all 12 must come back.

    python tools/time_hdbscan.py [--out profiles/hdbscan_timing.json] [--skip-host] [--skip-50k]
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
import hdbscan_ref as H  # noqa: E402

from speech_diarization_amd import cluster, hdbscan_gpu, ops  # noqa: E402

RATIO_BAR = 1.25


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


class TimedRows(hdbscan_gpu.DeviceRows):
    """DeviceRows with a pair of device events around every kernel pass."""

    def __init__(self, device):
        super().__init__(device)
        self.events = []

    def _timed(self, fn, *args):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(*args)
        b.record()
        self.events.append((a, b))
        return out

    def core(self, rows, k):
        return self._timed(super().core, rows, k)

    def outgoing(self, rows, core, comp):
        return self._timed(super().outgoing, rows, core, comp)

    def kernel_ms(self):
        torch.cuda.synchronize()
        return float(sum(a.elapsed_time(b) for a, b in self.events))


class TreeClock:
    """Wraps the two scikit-learn routines of `hdbscan_gpu._sklearn_tree` and adds up the seconds spent in them."""

    def __init__(self):
        self.dtype, self._mst, self._labels = hdbscan_gpu._sklearn_tree()
        self.seconds = 0.0

    def __call__(self):
        def timed(fn):
            def run(*args):
                t0 = time.perf_counter()
                out = fn(*args)
                self.seconds += time.perf_counter() - t0
                return out
            return run
        return self.dtype, timed(self._mst), timed(self._labels)


def kernel_cost(n, dev):
    X = torch.from_numpy(H.planted(n, 12, 0.5, 5, 0)).to(dev)
    Xn = ops.l2norm_rows(X, sklearn_zero_guard=True)
    ones = torch.ones(n, device=dev)
    singles = torch.arange(n, dtype=torch.int32, device=dev)
    op = hdbscan_gpu.DeviceRows(dev)
    reps = int(max(5, min(200, 4e10 / (float(n) * n))))
    core1 = op.core(Xn, 1)
    row = {"N": n, "d": int(Xn.shape[1]),
           "outgoing_singletons": event_ms(lambda: op.outgoing(Xn, core1, singles), reps),
           "ahc_nearest": event_ms(lambda: ops.ahc_nearest(Xn, ones, ws=op.ws), reps),
           "core_k1": event_ms(lambda: op.core(Xn, 1), reps), "core_k2": event_ms(lambda: op.core(Xn, 2), reps),
           "core_k16": event_ms(lambda: op.core(Xn, 16), max(2, reps // 4))}
    row["outgoing_over_ahc_nearest"] = row["outgoing_singletons"]["median_ms"] / row["ahc_nearest"]["median_ms"]
    row["ratio_bar"] = RATIO_BAR
    row["core_k2_over_outgoing"] = row["core_k2"]["median_ms"] / row["outgoing_singletons"]["median_ms"]
    row["outgoing_TFLOPs"] = float(n) * n * Xn.shape[1] / (row["outgoing_singletons"]["median_ms"] * 1e-3) / 1e12
    return row


def route(Xd, setting, metric, runs=5):
    total, kern, tree = [], [], []
    product_tree = hdbscan_gpu._sklearn_tree
    try:
        for it in range(runs + 1):                                    # the first one warms every shape up
            op, clock = TimedRows(Xd.device), TreeClock()
            hdbscan_gpu._sklearn_tree = clock
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            labels, info = hdbscan_gpu.hdbscan_rows(Xd, *setting, metric=metric, operator=op, return_info=True)
            t1 = time.perf_counter()
            if it:
                total.append((t1 - t0) * 1e3), kern.append(op.kernel_ms()), tree.append(clock.seconds * 1e3)
    finally:
        hdbscan_gpu._sklearn_tree = product_tree
    row = {"setting": list(setting), "metric": metric, "rounds": info["rounds"], "components_per_round": info["components_per_round"],
           "gram_rows_over_N2": info["gram_rows"] / float(Xd.shape[0]) ** 2, "total_ms": float(np.median(total)), "total_ms_min": float(min(total)),
           "total_ms_max": float(max(total)), "kernel_ms": float(np.median(kern)), "host_tree_ms": float(np.median(tree)),
           "clusters": int(len(set(labels.tolist()) - {-1})), "noise": int((labels < 0).sum())}
    row["device_share"] = row["kernel_ms"] / row["total_ms"]
    return labels, row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdbscan_timing.json"))
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-50k", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("time_hdbscan.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "host_cpus": os.environ.get("OMP_NUM_THREADS", "unset"), "kernels": [], "end_to_end": [],
           "scale": None}
    failures = []
    for n in (7609,) if a.skip_50k else (7609, 50000):
        row = kernel_cost(n, dev)
        res["kernels"].append(row)
        print(json.dumps(row), flush=True)
        if row["outgoing_over_ahc_nearest"] > RATIO_BAR:
            failures.append(f"one outgoing pass at N = {n} is {row['outgoing_over_ahc_nearest']:.2f} x the AHC nearest pass, the bar is {RATIO_BAR}")
        torch.cuda.empty_cache()

    n = 7609
    X = H.planted(n, 8, 0.8, 5, 40)
    Xd = torch.from_numpy(X).to(dev)
    for setting, metric in (((2, None, True), "euclidean"), ((6, 3, False), "cosine")):
        labels, row = route(Xd, setting, metric)
        row["N"] = n
        if not a.skip_host:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if metric == "euclidean":
                host = cluster.default_hdbscan_factory(min_cluster_size=setting[0], min_samples=setting[1], allow_single_cluster=setting[2],
                                                       metric="euclidean").fit_predict(X)
                row["host_call"] = "default_hdbscan_factory(metric='euclidean').fit_predict(rows)"
            else:
                host = cluster.hdbscan_precomputed(ops.cosine_affinity(Xd).cpu().numpy(), setting[0], None, setting[1], None)
                row["host_call"] = "affinity download + cluster.hdbscan_precomputed"
            row["host_s"] = time.perf_counter() - t0
            row["same_clustering"] = bool(H.same_clustering(labels, host))
            row["speedup"] = row["host_s"] / (row["total_ms"] * 1e-3)
            if row["speedup"] <= 1.0:
                failures.append(f"hdbscan_rows at {setting} is {row['speedup']:.2f} x the host route")
        res["end_to_end"].append(row)
        print(json.dumps(row), flush=True)
    if not a.skip_host:                                               # the two-stage glue of diarize(), either factory
        t0 = time.perf_counter()
        want = cluster.cluster_hdbscan_two_stage(X, 2)
        t1 = time.perf_counter()
        cluster.cluster_hdbscan_two_stage(X, 2, clusterer_factory=hdbscan_gpu.HdbscanGpuClusterer.factory())          # warm-up
        t2 = time.perf_counter()
        got = cluster.cluster_hdbscan_two_stage(X, 2, clusterer_factory=hdbscan_gpu.HdbscanGpuClusterer.factory())
        t3 = time.perf_counter()
        row = {"N": n, "call": "cluster.cluster_hdbscan_two_stage(rows, 2)", "host_s": t1 - t0, "device_s": t3 - t2,
               "speedup": (t1 - t0) / (t3 - t2), "same_clustering": bool(H.same_clustering(got, want))}
        res["end_to_end"].append(row)
        print(json.dumps(row), flush=True)
        if row["speedup"] <= 1.0:
            failures.append(f"the two-stage glue on the device route is {row['speedup']:.2f} x the host route")
    del Xd
    torch.cuda.empty_cache()

    if not a.skip_50k:
        n, k = 50000, 12
        r = np.random.default_rng(5)                                   # planted()'s draw order: its labels are the second draw
        r.standard_normal((k, 192))
        planted = r.integers(0, k, n)
        Xd = torch.from_numpy(H.planted(n, k, 0.5, 5, 0)).to(dev)
        setting = (15, 5, True)
        hdbscan_gpu.hdbscan_rows(Xd[:4096], *setting)                  # warm-up at another size
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        op = TimedRows(dev)
        labels, info = hdbscan_gpu.hdbscan_rows(Xd, *setting, operator=op, return_info=True)
        wall = time.perf_counter() - t0
        found = sorted(set(labels.tolist()) - {-1})
        owners = {int(np.bincount(planted[labels == c], minlength=k).argmax()) for c in found}
        pure = all(len(set(planted[labels == c].tolist())) == 1 for c in found)
        res["scale"] = {"N": n, "planted_speakers": k, "setting": list(setting), "wall_s": wall, "kernel_ms": op.kernel_ms(), "rounds": info["rounds"],
                        "components_per_round": info["components_per_round"], "clusters": len(found), "noise": int((labels < 0).sum()),
                        "all_speakers_recovered": bool(len(found) == k and len(owners) == k and pure)}
        print(json.dumps(res["scale"]), flush=True)
        if not res["scale"]["all_speakers_recovered"]:
            failures.append(f"{len(found)} clusters for {k} planted speakers at N = {n}")
    res["failures"] = failures
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    if failures:
        raise SystemExit("; ".join(failures))


if __name__ == "__main__":
    main()
