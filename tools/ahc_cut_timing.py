"""Time the bounded AHC route (speaker-count bounds by a dendrogram cut on the device) on the GPU -> profiles/ahc_cut_timing.json.

For folders of R planted recordings of m rows each, (R, m) in {(256, 500), (1024, 200), (16, 7609)} (8 planted speakers, as
tools/ahc_grouped_timing.py), host clock around calls that end in a host result, the variants alternating in one process: median, min
and max of 5 runs each after a warm-up of all:
* (a) `ahc_gpu.ahc_cosine_groups` without bounds at cosine 0.3: the parent's code;
* (b) the same with bounds that do not bind (min 1, max m): the difference from (a) is the merge log and one launch of the cut;
* (c) bounds that bind at the maximum for every recording, twice: at 0.3 with max 4 (the threshold leaves the 8 planted clusters,
  phase B merges them on), and at 0.9 with min = max = 8 (the threshold leaves hundreds of clusters per recording, phase B builds
  most of the dendrogram); the rounds of phase B are recorded;
* the cut launch alone on the log of (c, 0.9) (device events, 20 launches per window);
* for scale, the host route the feature replaces: scipy `linkage(squareform(D), "average")` + `fcluster(Z, 8, "maxclust")` per
  recording from its N x N cosine matrix, timed on a few recordings of the folder and reported per recording.
No bar: nothing here was measured before.

    python tools/ahc_cut_timing.py [--out profiles/ahc_cut_timing.json] [--cases 256x500,1024x200,16x7609]
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

from speech_diarization_amd import ahc_gpu  # noqa: E402

COS_THR, STRICT_THR, SPEAKERS = 0.3, 0.9, 8
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


class KeepsLog(ahc_gpu.DeviceSums):
    """DeviceSums that keeps what `cut` was handed."""

    def cut(self, *args):
        self.seen = args
        return super().cut(*args)


def host_route_ms(parts, recordings):
    """scipy's average linkage and the cut into SPEAKERS per recording from its N x N f64 distance matrix."""
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    ms = []
    for x in parts[:recordings]:
        xn = x / np.linalg.norm(x, axis=1, keepdims=True)
        t0 = time.perf_counter()
        D = 1.0 - (xn @ xn.T).astype(np.float64)
        D = 0.5 * (D + D.T)
        np.fill_diagonal(D, 0.0)
        np.clip(D, 0.0, None, out=D)
        fcluster(linkage(squareform(D, checks=False), "average"), SPEAKERS, "maxclust")
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def case(dev, n_rec, m):
    parts = [R.planted_rows(m, SPEAKERS, 0.5, 1000 * n_rec + s, dtype=np.float32)[0] for s in range(n_rec)]
    Xd = torch.from_numpy(np.concatenate(parts)).to(dev)
    sizes = [m] * n_rec
    op = KeepsLog(dev)
    variants = {
        "a_unbounded": lambda: ahc_gpu.ahc_cosine_groups(Xd, sizes, COS_THR, operator=op, return_info=True),
        "b_bounds_that_do_not_bind": lambda: ahc_gpu.ahc_cosine_groups(Xd, sizes, COS_THR, operator=op, return_info=True, min_clusters=1, max_clusters=m),
        "c_max_4_at_0.3": lambda: ahc_gpu.ahc_cosine_groups(Xd, sizes, COS_THR, operator=op, return_info=True, min_clusters=1, max_clusters=4),
        "c_known_8_at_0.9": lambda: ahc_gpu.ahc_cosine_groups(Xd, sizes, STRICT_THR, operator=op, return_info=True, min_clusters=SPEAKERS,
                                                              max_clusters=SPEAKERS),
    }
    first = {name: fn() for name, fn in variants.items()}              # the warm-up of all, and what they return
    ms = {name: [] for name in variants}
    for _ in range(RUNS):                                              # alternating: other work shares the host
        for name, fn in variants.items():
            ms[name].append(wall_ms(fn)[0])
    row = {"recordings": n_rec, "rows_each": m, "rows": n_rec * m}
    for name, (labels, info) in first.items():
        row[name] = {"ms": stats(ms[name]), "rounds": info["rounds"], "rounds_full": info.get("rounds_full", 0),
                     "clusters_min_max": [int(min(info["clusters"])), int(max(info["clusters"]))]}
        if "threshold_clusters" in info:
            row[name]["threshold_clusters_min_max"] = [int(min(info["threshold_clusters"])), int(max(info["threshold_clusters"]))]
    row["b_same_labels_as_a"] = bool(all(np.array_equal(g, w) for g, w in zip(first["b_bounds_that_do_not_bind"][0], first["a_unbounded"][0])))
    row["b_minus_a_ms_median"] = row["b_bounds_that_do_not_bind"]["ms"]["median"] - row["a_unbounded"]["ms"]["median"]
    variants["c_known_8_at_0.9"]()                                     # its log is the one the cut is timed on
    seen = op.seen
    row["cut_alone"] = {"merges": int(seen[2].numel()), "ms": stats(event_ms(lambda: ahc_gpu.DeviceSums.cut(op, *seen)))}
    timed = min(n_rec, 4 if m <= 1000 else 1)
    host = host_route_ms(parts, timed)
    row["host_scipy_per_recording_ms"] = {"recordings_timed": timed, **stats(host)}
    row["host_scipy_folder_ms_extrapolated"] = float(np.median(host) * n_rec)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ahc_cut_timing.json"))
    ap.add_argument("--cases", default="256x500,1024x200,16x7609")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("ahc_cut_timing.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "cos_thr": COS_THR, "strict_thr": STRICT_THR, "runs": RUNS,
           "host_cpus": os.environ.get("OMP_NUM_THREADS", "unset"), "cases": []}
    for n_rec, m in [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",") if c]:
        res["cases"].append(case(dev, n_rec, m))
        print(json.dumps(res["cases"][-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
