"""Measure the rounding error of sd_affinity_apply_f32 / sd_affinity_degree_f32 over the shape grid of tests/test_gpu_spectral.py
against the f64 numpy reference, on the GPU, and write profiles/spectral_accuracy.json (the file the test's bar quotes).

    python tools/spectral_accuracy.py [--out profiles/spectral_accuracy.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import spectral_ref as R  # noqa: E402

from speech_diarization_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_accuracy.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows, worst, worst_deg = [], 0.0, 0.0
    for n in R.GRID_N:
        for ld in R.grid_lds(n):
            Kp = R.grid_affinity(n, ld, seed=n)
            Kd = torch.from_numpy(Kp).to(dev)[:, :n]
            K = Kp[:, :n]
            for zd in (False, True):
                ref = R.degree_ref(K, zd)
                deg = ops.affinity_degree(Kd, zd).cpu().numpy().astype(np.float64)
                rel = float(np.max(np.abs(deg - ref) / np.where(ref > 0, ref, 1.0)))
                worst_deg = max(worst_deg, rel)
                scale = R.grid_scale(K, zd)
                for b in R.GRID_B:
                    V = R.grid_block(n, b, seed=n + b)
                    Y = ops.affinity_apply(Kd, torch.from_numpy(scale).to(dev), torch.from_numpy(V).to(dev), zd).cpu().numpy()
                    r = R.apply_error_over_bound(Y, K, scale, V, zd)
                    worst = max(worst, r)
                    rows.append({"N": n, "ld": ld, "zero_diag": zd, "b": b, "error_over_bound": r, "degree_rel_err": rel})
    out = {
        "what": "max |Y - Y64| / (N 2^-23 (|S| |V|)) of sd_affinity_apply_f32 and max relative error of sd_affinity_degree_f32 "
                "against f64 numpy over the grid of tests/test_gpu_spectral.py",
        "device": torch.cuda.get_device_name(0),
        "apply_max_error_over_bound": worst,
        "degree_max_rel_err": worst_deg,
        "cases": rows,
    }
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("device", "apply_max_error_over_bound", "degree_max_rel_err")}))


if __name__ == "__main__":
    main()
