"""Time HDBSCAN's labelling on the device against the scikit-learn tail, in the same run -> profiles/hdbscan_labels_timing.json.

The folders of tools/hdbscan_grouped_timing.py, R planted recordings of m rows each, (R, m) in {(256, 500), (1024, 200), (16, 7609)}
(`hdbscan_ref.planted`: 8 speakers, noise 0.8, one row in 50 an outlier), at (min_cluster_size, min_samples) = (2, None) and (6, 3):
* TO THE LABELS: `hdbscan_rows_groups(..., labelling="sklearn")` (the parent's behaviour, and the default) against
  `labelling="device"`, over rows that are already on the device;
* THE LABELLING STEP ALONE on the edge lists of one `spanning_edges_groups`: the loop of `_labels_of_tree` (scikit-learn's
  `_process_mst` + `tree_to_labels` per recording) against `_labels_on_device` (one upload, one `sd_tree_labels_grouped` launch, one
  read), and the launch by itself (device events over edges that are already up).
Host clock around calls that end in a host result, the two routes alternating in one process: minimum, median and maximum of 5 runs
each after a warm-up of both.  Whether the two labellings agree is recorded per case (they must wherever no two distances of a
recording tie; at (6, 3) ties are the rule, hdbscan_gpu's docstring), never asserted here.

The bar, against the scikit-learn route of the same run: at (256, 500) and (2, None) the MAXIMUM of the device route to the labels is
at most half the MINIMUM of the scikit-learn route.  At (16, 7609) the one-lane sections of the kernel run over state in global memory
and dominate; that case is recorded whatever it shows.

    python tools/hdbscan_labels_timing.py [--out profiles/hdbscan_labels_timing.json] [--cases 256x500,1024x200]
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

from speech_diarization_amd import _native, hdbscan_gpu  # noqa: E402

SETTINGS = ((2, None), (6, 3))
BAR_CASE, BAR_SETTING, BAR = (256, 500), (2, None), 2.0
RUNS = 5


def stats(ms):
    return {"min": float(min(ms)), "median": float(np.median(ms)), "max": float(max(ms))}


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def event_ms(fn, reps=5, windows=RUNS, warmup=2):
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


def case(dev, n_rec, m, setting):
    mcs, ms = setting
    k = (mcs if ms is None else ms) - 1
    parts = [H.planted(m, 8, 0.8, 1000 * n_rec + s, m // 50) for s in range(n_rec)]
    Xd = torch.from_numpy(np.concatenate(parts)).to(dev)
    sizes = [m] * n_rec
    op = hdbscan_gpu.DeviceRows(dev)
    sk = hdbscan_gpu._sklearn_tree()

    def to_labels(labelling):
        return hdbscan_gpu.hdbscan_rows_groups(Xd, sizes, mcs, ms, operator=op, labelling=labelling)

    rows = op.normalise(Xd)
    group = torch.arange(n_rec, dtype=torch.int32, device=dev).repeat_interleave(m)
    core, bad = op.core_grouped(rows, k, group, m)
    edges = hdbscan_gpu.spanning_edges_groups(rows, core, sizes, op, None, bad)

    def step_sklearn():
        return [hdbscan_gpu._labels_of_tree(lo, hi, w, m, mcs, True, "euclidean", sk)[0] for lo, hi, w in edges]

    def step_device():
        return hdbscan_gpu._labels_on_device(edges, mcs, True, "euclidean", op)[0]

    want, got = to_labels("sklearn"), to_labels("device")             # the warm-up of both, and the comparison
    step_want, step_got = step_sklearn(), step_device()
    t = {"sk": [], "dev": [], "step_sk": [], "step_dev": []}
    for _ in range(RUNS):                                             # alternating: other work shares the host
        t["sk"].append(wall_ms(lambda: to_labels("sklearn"))[0])
        t["dev"].append(wall_ms(lambda: to_labels("device"))[0])
    for _ in range(RUNS):
        t["step_sk"].append(wall_ms(step_sklearn)[0])
        t["step_dev"].append(wall_ms(step_device)[0])
    # the launch by itself, over edges that are already on the device
    counts = np.array([len(w) for _, _, w in edges])
    lo = torch.from_numpy(np.concatenate([e[0] for e in edges]).astype(np.int32)).to(dev)
    hi = torch.from_numpy(np.concatenate([e[1] for e in edges]).astype(np.int32)).to(dev)
    dist = torch.from_numpy(np.concatenate([hdbscan_gpu._tree_distances(e[2], "euclidean") for e in edges])).to(dev)
    first = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dev)
    launch = event_ms(lambda: op.tree_labels(lo, hi, dist, first, int(counts.max()), mcs, True))
    tied = sum(int(len(np.unique(hdbscan_gpu._tree_distances(e[2], "euclidean"))) < len(e[2])) for e in edges)
    E = int(counts.sum())
    row = {"recordings": n_rec, "rows_each": m, "rows": n_rec * m, "min_cluster_size": mcs, "min_samples": ms,
           "to_labels_sklearn_ms": stats(t["sk"]), "to_labels_device_ms": stats(t["dev"]),
           "to_labels_sklearn_min_over_device_max": min(t["sk"]) / max(t["dev"]),
           "to_labels_sklearn_median_over_device_median": float(np.median(t["sk"]) / np.median(t["dev"])),
           "labelling_sklearn_ms": stats(t["step_sk"]), "labelling_device_ms": stats(t["step_dev"]),
           "labelling_sklearn_median_over_device_median": float(np.median(t["step_sk"]) / np.median(t["step_dev"])),
           "launch_ms": stats(launch), "state": "LDS" if m <= (160 * 1024 - 256) // 72 else "workspace",
           "workspace_bytes": int(_native.load().sd_tree_labels_workspace_bytes(E, n_rec, int(counts.max()))),
           "recordings_with_tied_distances": tied,
           "same_labels_to_labels": bool(all(np.array_equal(g, w) for g, w in zip(got, want))),
           "same_labels_step": bool(all(np.array_equal(g, w) for g, w in zip(step_got, step_want))),
           "recordings_that_differ": int(sum(not np.array_equal(g, w) for g, w in zip(step_got, step_want)))}
    if (n_rec, m) == BAR_CASE and setting == BAR_SETTING:
        row["bar"] = BAR
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdbscan_labels_timing.json"))
    ap.add_argument("--cases", default="256x500,1024x200,16x7609")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("hdbscan_labels_timing.py measures on the GPU; there is nothing to time without one")
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "runs": RUNS, "host_cpus": os.environ.get("OMP_NUM_THREADS", "unset"), "cases": []}
    for n_rec, m in [tuple(int(v) for v in c.split("x")) for c in a.cases.split(",") if c]:
        for setting in SETTINGS:
            res["cases"].append(case(dev, n_rec, m, setting))
            print(json.dumps(res["cases"][-1]), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    bar = [r for r in res["cases"] if "bar" in r]
    if bar and bar[0]["to_labels_sklearn_min_over_device_max"] < BAR:
        raise SystemExit(f"to the labels at {BAR_CASE}: the scikit-learn route is {bar[0]['to_labels_sklearn_min_over_device_max']:.2f} x the "
                         f"device route, the bar is {BAR} x")


if __name__ == "__main__":
    main()
