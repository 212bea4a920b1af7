"""Time the grouped HDBSCAN route against one driver per recording on the GPU -> profiles/hdbscan_grouped_timing.json.

For folders of R planted recordings of m rows each, (R, m) in {(64, 500), (256, 500), (1024, 200), (16, 7609)} (`hdbscan_ref.planted`:
8 speakers, noise 0.8, one row in 50 an outlier), at (min_cluster_size, min_samples) = (2, None) (what `diarize()` passes) and (6, 3) (diar_diag's):
* the TREE STAGE, the core pass plus Boruvka up to the edge lists, over unit rows that are already on the device:
  `operator.core_grouped` + `hdbscan_gpu.spanning_edges_groups` over the folder against the loop of `operator.core` +
  `hdbscan_gpu.spanning_edges` over its recordings (the baseline: the parent's driver).  Host clock around calls that end in a host
  result, the two alternating in one process: median, min and max of 5 runs each after a warm-up of both;
* END TO END to the labels, recorded without a bar: `hdbscan_rows_groups` against the loop of `hdbscan_rows`.  The per-recording
  scikit-learn labelling is the same host work in both and is part of both figures;
* rounds of both (the loop's sum and maximum), the first grouped pass alone (device events), the tiles over all passes, the workspace
  bytes of both, and that both routes return the same edge lists and the same labels.
The bar, on the tree stage only: at (256, 500) and (2, None) the loop's minimum over the grouped maximum is at least 4.  The per-step
split of the grouped tree stage at that size (core pass, outgoing passes, and what the host does between them; a synchronise after
each pass, so their sum exceeds the unsynchronised run) is recorded beside it.

    python tools/hdbscan_grouped_timing.py [--out profiles/hdbscan_grouped_timing.json] [--cases 64x500,256x500]
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
BAR_CASE, BAR_SETTING, BAR = (256, 500), (2, None), 4.0
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


class SteppedRows(hdbscan_gpu.DeviceRows):
    """DeviceRows that synchronises after every grouped pass and books the host time by step; what the driver does between two passes
    (the read-back, the edge selection, the components, the upload of `comp`) is booked from the gaps."""

    def __init__(self, device):
        super().__init__(device)
        self.ms = {"core": 0.0, "outgoing": 0.0, "host_between_passes": 0.0}
        self.left = None

    def _timed(self, key, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if self.left is not None:
            self.ms["host_between_passes"] += (t0 - self.left) * 1e3
        out = fn()
        torch.cuda.synchronize()
        self.left = time.perf_counter()
        self.ms[key] += (self.left - t0) * 1e3
        return out

    def core_grouped(self, rows, k, group, max_group):
        return self._timed("core", lambda: super(SteppedRows, self).core_grouped(rows, k, group, max_group))

    def outgoing_grouped(self, rows, core, comp, group, max_group):
        return self._timed("outgoing", lambda: super(SteppedRows, self).outgoing_grouped(rows, core, comp, group, max_group))


def case(dev, n_rec, m, setting):
    lib = _native.load()
    mcs, ms = setting
    k = (mcs if ms is None else ms) - 1
    parts = [H.planted(m, 8, 0.8, 1000 * n_rec + s, m // 50) for s in range(n_rec)]
    Xd = torch.from_numpy(np.concatenate(parts)).to(dev)
    sizes = [m] * n_rec
    op_g, op_l = hdbscan_gpu.DeviceRows(dev), hdbscan_gpu.DeviceRows(dev)
    rows = op_g.normalise(Xd)
    each_rows = [rows[i * m:(i + 1) * m] for i in range(n_rec)]
    each_X = [Xd[i * m:(i + 1) * m] for i in range(n_rec)]
    group = torch.arange(n_rec, dtype=torch.int32, device=dev).repeat_interleave(m)

    def tree_grouped(op=op_g, info=None):
        core, bad = op.core_grouped(rows, k, group, m)
        return hdbscan_gpu.spanning_edges_groups(rows, core, sizes, op, info, bad)

    def tree_loop(infos=None):
        out = []
        for r in each_rows:
            info = {"rounds": 0, "gram_rows": 0, "components_per_round": []} if infos is not None else None
            out.append(hdbscan_gpu.spanning_edges(r, op_l.core(r, k), op_l, info))
            if infos is not None:
                infos.append(info)
        return out

    def labels_grouped():
        return hdbscan_gpu.hdbscan_rows_groups(Xd, sizes, mcs, ms, operator=op_g)

    def labels_loop():
        return [hdbscan_gpu.hdbscan_rows(x, mcs, ms, operator=op_l) for x in each_X]

    got, want = tree_grouped(), tree_loop()                           # the warm-up of both, and the comparison
    same_edges = all(np.array_equal(a, b) for g, w in zip(got, want) for a, b in zip(g, w))
    got_l, want_l = labels_grouped(), labels_loop()
    t = {"tree_g": [], "tree_l": [], "lab_g": [], "lab_l": []}
    for _ in range(RUNS):                                             # alternating: other work shares the host
        t["tree_g"].append(wall_ms(tree_grouped)[0])
        t["tree_l"].append(wall_ms(tree_loop)[0])
    for _ in range(RUNS):
        t["lab_g"].append(wall_ms(labels_grouped)[0])
        t["lab_l"].append(wall_ms(labels_loop)[0])
    infos = []
    tree_loop(infos)
    rounds = [i["rounds"] for i in infos]
    _, info = hdbscan_gpu.hdbscan_rows_groups(Xd, sizes, mcs, ms, operator=op_g, return_info=True)
    first = event_ms(lambda: op_g.core_grouped(rows, k, group, m))
    d = rows.shape[1]
    n = n_rec * m
    row = {"recordings": n_rec, "rows_each": m, "rows": n, "min_cluster_size": mcs, "min_samples": ms, "k": k,
           "tree_grouped_ms": stats(t["tree_g"]), "tree_loop_ms": stats(t["tree_l"]),
           "tree_loop_min_over_grouped_max": min(t["tree_l"]) / max(t["tree_g"]),
           "tree_loop_median_over_grouped_median": float(np.median(t["tree_l"]) / np.median(t["tree_g"])),
           "labels_grouped_ms": stats(t["lab_g"]), "labels_loop_ms": stats(t["lab_l"]),
           "labels_loop_median_over_grouped_median": float(np.median(t["lab_l"]) / np.median(t["lab_g"])),
           "rounds_grouped": info["rounds"], "rounds_loop_sum": int(sum(rounds)), "rounds_loop_max": int(max(rounds)),
           "host_synchronisations_grouped": info["rounds"], "host_synchronisations_loop": int(sum(rounds)),
           "gram_tiles_all_passes": info["gram_tiles"], "gram_tiles_per_pass": info["gram_tiles_per_pass"],
           "first_grouped_pass_ms": stats(first),
           "workspace_bytes_grouped": {"core": int(lib.sd_hdb_core_grouped_workspace_bytes(n, d, k, m)),
                                       "outgoing": int(lib.sd_hdb_outgoing_grouped_workspace_bytes(n, d, m))},
           "workspace_bytes_loop": {"core": int(lib.sd_hdb_core_workspace_bytes(m, d, k)), "outgoing": int(lib.sd_hdb_outgoing_workspace_bytes(m, d))},
           "workspace_bytes_ungrouped_over_all_rows": {"core": int(lib.sd_hdb_core_workspace_bytes(n, d, k)),
                                                       "outgoing": int(lib.sd_hdb_outgoing_workspace_bytes(n, d))},
           "same_edges": bool(same_edges), "same_labels": bool(all(np.array_equal(g, w) for g, w in zip(got_l, want_l)))}
    if (n_rec, m) == BAR_CASE and setting == BAR_SETTING:
        step = SteppedRows(dev)
        tree_grouped(step)                                            # its own warm-up (a workspace of its own)
        step.ms, step.left = {key: 0.0 for key in step.ms}, None
        tree_grouped(step)
        row["grouped_tree_split_ms_synchronised"] = dict(step.ms)
        row["bar"] = BAR
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hdbscan_grouped_timing.json"))
    ap.add_argument("--cases", default="64x500,256x500,1024x200,16x7609")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("hdbscan_grouped_timing.py measures on the GPU; there is nothing to time without one")
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
    if bar and bar[0]["tree_loop_min_over_grouped_max"] < BAR:
        raise SystemExit(f"the grouped tree stage at {BAR_CASE} is {bar[0]['tree_loop_min_over_grouped_max']:.2f} x the loop, the bar is {BAR} x")


if __name__ == "__main__":
    main()
