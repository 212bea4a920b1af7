#!/usr/bin/env python3
"""What the ECAPA forward launches and computes, as a record two libraries can be diffed on (a host-only change to the schedule
must leave every entry as it was: same kernels in the same order on the same inputs give the same bits).

    python tools/forward_census.py --out FILE [--sizes-only]          one record, of the library this process loads
    python tools/forward_census.py --diff PARENT.json NEW.json --summary profiles/ecapa_plan_parity.json

A record holds, for every forward of tests/helpers/ecapa_plan.census_cases() (four precisions, both f16_tiles settings, uniform /
relative-length / packed maps, the shapes of the GPU test plus both sides of the small-launch edges): the launch log as label ->
count, the SHA-256 of the embedding bytes and the workspace size; and, over the whole CPU sweep of tests/test_ecapa_plan_rules.py,
sd_ecapa_workspace_bytes(B, T) and sd_ecapa_packed_workspace_bytes(B, B * T).  --sizes-only writes the second half alone (no GPU).

Run it once per library, each in a process of its own: the library under test is the tree's, another one (the parent's, built from a
checkout outside the tree into speech-diarization_amd/variants/) comes in with SD_EXPERIMENT=1 SD_HIP_LIB=<path>.  An older library
lacks the newer entries of the trace header; the binding table is cut down to what it exports.  --diff compares two records entry by
entry with no tolerance and writes the summary: the parent's record, and for each entry whether the new one is identical."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))

SWEEP_B = (1, 2, 35, 36, 40, 41, 44, 256, 257)
SWEEP_T = (7, 61, 63, 64, 127, 128, 129, 201)


def bind_what_the_library_has():
    """SD_HIP_LIB names an older build: keep the trace entries it exports and take its trace version as the expected one."""
    import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch has loaded, as in every other process of the project)
    from speech_diarization_amd import _native as N
    path = os.environ.get("SD_HIP_LIB")
    if path and os.environ.get("SD_EXPERIMENT") == "1":
        lib = C.CDLL(path)
        N.TRACE_PROTOTYPES = {k: v for k, v in N.TRACE_PROTOTYPES.items() if hasattr(lib, k)}
        N.SD_TRACE_ABI_VERSION = lib.sd_trace_abi_version()
    return N


def workspace_sweep(N):
    import ecapa_plan as P
    lib = N.load()
    out = {}
    for geom in P.GEOMETRIES:
        for prec in P.PRECISIONS:
            W = C.byref(P.cpu_weights(geom, prec).struct)
            for B in SWEEP_B:
                for T in SWEEP_T:
                    out[f"{geom}-{prec}-B{B}-T{T}"] = [int(lib.sd_ecapa_workspace_bytes(W, B, T)), int(lib.sd_ecapa_packed_workspace_bytes(W, B, B * T))]
    return out


def forwards(N):
    import torch
    import ecapa_plan as P
    import launch_log as L
    from speech_diarization_amd.engine import EmbeddingEngine
    dev = torch.device("cuda", 0)
    engines, out = {}, {}
    for case in P.census_cases():
        key = (case.geom, case.precision)
        if key not in engines:
            engines[key] = EmbeddingEngine(P.state_dict(case.geom), dev, precision=case.precision)
        eng = engines[key]
        P.set_tiles(case.tiles)
        try:
            with L.launches() as log:
                emb = P.run_case(case, eng)
            torch.cuda.synchronize()
        finally:
            P.set_tiles("auto")
        W = C.byref(eng.weights.struct)
        if case.kind == "packed":
            ws = int(eng._lib.sd_ecapa_packed_workspace_bytes(W, len(case.spans), sum(P.frames(n) for n in case.spans)))
        else:
            ws = int(eng._lib.sd_ecapa_workspace_bytes(W, case.B, P.frames(case.n)))
        out[case.id] = {"launches": dict(sorted(log.items())), "sha256": hashlib.sha256(emb.cpu().numpy().tobytes()).hexdigest(),
                        "finite": bool(torch.isfinite(emb).all()), "workspace_bytes": ws}
    return out


def record(a):
    N = bind_what_the_library_has()
    N.load()
    variant = os.environ.get("SD_HIP_LIB") if os.environ.get("SD_EXPERIMENT") == "1" else None
    rec = {"library": os.path.relpath(os.path.abspath(variant or str(N.LIB_PATH)), ROOT),
           "trace_abi": int(N.load().sd_trace_abi_version()), "workspace": workspace_sweep(N)}
    if not a.sizes_only:
        rec["forwards"] = forwards(N)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"{len(rec.get('forwards', {}))} forwards, {len(rec['workspace'])} workspace sizes -> {a.out}")
    return 0


def diff(a):
    old, new = (json.load(open(p)) for p in a.diff)
    differing = []
    for part in ("forwards", "workspace"):
        keys = sorted(set(old.get(part, {})) | set(new.get(part, {})))
        differing += [f"{part}: {k}" for k in keys if old.get(part, {}).get(k) != new.get(part, {}).get(k)]
    commit = lambda rev: subprocess.run(["git", "rev-parse", rev], cwd=ROOT, capture_output=True, text=True).stdout.strip()  # noqa: E731
    rec = {"parent": {"commit": a.parent_commit or commit("HEAD"), "library": old["library"], "trace_abi": old["trace_abi"]},
           "new": {"library": new["library"], "trace_abi": new["trace_abi"]},
           "summary": {"forwards": len(old.get("forwards", {})), "workspace_sizes": len(old.get("workspace", {})),
                       "identical": len(old.get("forwards", {})) + len(old.get("workspace", {})) - len(differing), "differing": differing},
           "forwards": old.get("forwards", {}), "workspace": old.get("workspace", {})}
    with open(a.summary, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for d in differing:
        print("DIFFERS", d)
    print(f"{rec['summary']['identical']} entries identical, {len(differing)} differ -> {a.summary}")
    return 1 if differing or not old.get("forwards") else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="where the record of this library goes")
    ap.add_argument("--sizes-only", action="store_true", help="the workspace sweep alone (no GPU)")
    ap.add_argument("--diff", nargs=2, metavar=("PARENT", "NEW"), help="compare two records")
    ap.add_argument("--summary", default=os.path.join(ROOT, "profiles", "ecapa_plan_parity.json"))
    ap.add_argument("--parent-commit", default=None, help="the commit of the PARENT record (default: HEAD, for an uncommitted change)")
    a = ap.parse_args()
    sys.exit(diff(a) if a.diff else record(a))
