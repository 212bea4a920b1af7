#!/usr/bin/env python3
"""Which kernel every conv entry takes, over one list of shapes, as a record two libraries can be diffed on.  A library that predates
the choice layer (csrc/sd_conv_choice.h) can only be ASKED by launching, one that has it can be read:

    python tools/conv_choice_census.py --launch --out FILE     GPU: launch every shape of the list, record the launch log
    python tools/conv_choice_census.py --read --out FILE       sd_conv_choice_read for the same list and --n-cu CUs (default 256); no launch
    python tools/conv_choice_census.py --diff LAUNCHED.json READ.json [--bench RUNS.json] [--forwards FWD.json] --summary profiles/conv_choice_parity.json

The parent's library comes in with SD_EXPERIMENT=1 SD_HIP_LIB=<its build under speech-diarization_amd/variants/>, one process per
library (tools/forward_census.py).  The list: the runs of tests/test_gpu_exact.py::test_the_choice_is_what_ran (tests/helpers/
conv_choice.CHOICE_RUNS), and every conv of the full geometry (80 mels, C = 1024, 3C = 3072, Res2Net scale 8, attention 128, T = 201) at
B in {1, 16, 32, 40, 41, 64, 300} through each entry that takes it: under the shipped tuning, under every f32 pin at B = 16 and 300, and
under both settings of SD_TUNE_F16_NARROW_TILES and SD_TUNE_T256_LOCKSTEP_TILES.  The largest launch is the 3C -> 3C conv over 60 300 rows,
far below one launch of the 10 000-segment forward.  Operands are zeros: the record is the labels, not the numbers.

--diff: every shape must have the same labels in both records; --bench adds the six alternated bench.py runs (a JSON list of
{"library", "value", "numpy_batch32"}) with the medians and the parent's spread, --forwards the summary of `forward_census.py --diff`."""
import argparse
import collections
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

BATCHES = (1, 16, 32, 40, 41, 64, 300)
T = 201
# the convs of the full geometry: name -> (cin, cout, taps, dil, what the epilogue carries)
LAYERS = {
    "stem": (80, 1024, 5, 1, ""), "tdnn1": (1024, 1024, 1, 1, "tee"), "tdnn2": (1024, 1024, 1, 1, ""), "tdnn2+stat": (1024, 1024, 1, 1, "colstat"),
    "res2.d2": (128, 128, 3, 2, "tee_add"), "res2.d3": (128, 128, 3, 3, "tee_add"), "res2.d4": (128, 128, 3, 4, "tee_add"),
    "mfa": (3072, 3072, 1, 1, ""), "mfa+stat": (3072, 3072, 1, 1, "colstat"), "asp_h": (3072, 128, 1, 1, "per_seg"), "asp_conv": (128, 3072, 1, 1, ""),
}
SEG_LAYERS = {"se1": (1024, 128), "se2": (128, 1024), "asp_g": (6144, 128), "fc": (6144, 192)}
NARROW = ("res2.d2", "res2.d3", "res2.d4", "asp_h")
WIDE = ("stem", "tdnn1", "tdnn2", "tdnn2+stat", "mfa", "mfa+stat", "asp_conv")


def shape_list():
    """[(id, op, kwargs of conv_choice.conv_args, selection, {tuning key: value})], the same list for --launch and --read."""
    import conv_choice as CC
    from kernel_selection import CONV_KERNELS
    out = []
    for runs in CC.CHOICE_RUNS.values():
        for op, shape, sel, tune in runs:
            s = CC.CHOICE_SHAPES[shape]
            M = sum(s["spans"]) if "spans" in s else s["B"] * s["T"]
            kw = dict(M=M, T=M if "spans" in s else s["T"], cin=s["cin"], cout=s["cout"], taps=s["k"], dil=s["dil"])
            dt = dict(x=CC.F16 if tune.get("x16") else CC.F32, y=CC.F16 if tune.get("y16") else CC.F32) if op == "f16" else {}
            out.append((f"test/{op}/{shape}/{sel}/{sorted(tune.items())}", op, {**kw, **dt}, sel, {k: v for k, v in tune.items() if k in ("f16_tiles", "lockstep")}))
    for B in BATCHES:
        for name, (cin, cout, taps, dil, epi) in LAYERS.items():
            kw = dict(M=B * T, T=T, cin=cin, cout=cout, taps=taps, dil=dil, colstat=epi == "colstat", bias_per_seg=epi == "per_seg",
                      act2="tanh" if epi == "per_seg" else None, tee=(128, 256) if epi == "tee" else (0, 128) if epi == "tee_add" else None, tee_add=epi == "tee_add")
            for sel in CONV_KERNELS if B in (16, 300) else ("auto",):
                out.append((f"full/f32/{name}/B{B}/{sel}", "f32", kw, sel, {}))
            if taps > 1 or epi == "per_seg":
                out.append((f"full/packed/{name}/B{B}", "packed", {**kw, "T": B * T, "colstat": False}, "auto", {}))
            for tiles in (-1, 0):
                for lockstep in (-1, 0):
                    tune = dict(f16_tiles=tiles, lockstep=lockstep)
                    for x16, y16 in ((1, 1), (1, 0)) if name != "stem" else ((1, 1), (0, 1)):
                        out.append((f"full/f16/{name}/B{B}/x{x16}y{y16}/{tiles}/{lockstep}", "f16", {**kw, "x": CC.F16 if x16 else CC.F32, "y": CC.F16 if y16 else CC.F32}, "auto", tune))
                    if name in WIDE and not (epi == "tee"):
                        out.append((f"full/wide/{name}/B{B}/{tiles}/{lockstep}", "wide", kw, "auto", tune))
                        if not kw["colstat"]:
                            out.append((f"full/wide/{name}/B{B}/{tiles}/{lockstep}/split_out", "wide", {**kw, "y": CC.SPLIT}, "auto", tune))
            if name in NARROW:
                out.append((f"full/narrow/{name}/B{B}", "narrow", kw, "auto", {}))
        for name, (cin, cout) in SEG_LAYERS.items():
            out.append((f"full/seg/{name}/B{B}", "seg", dict(M=B, T=1, cin=cin, cout=cout, act=None), "auto", {}))
    assert len({e[0] for e in out}) == len(out)
    return out


def build_args(op, kw, lib):
    """conv_choice.conv_args for one entry of the list, with the operator's dtypes and granularities; -> (entry op of CONV_OPS, args, scratch bytes)."""
    import conv_choice as CC
    kw = dict(kw)
    cin = kw["cin"]
    if op == "f16":
        return "f16", CC.conv_args(cin_pad=-(-cin // 64) * 64, w=CC.F16, **kw), 0
    if op == "narrow":
        return "split16", CC.conv_args(w=CC.SPLIT, **{**kw, "ldo": -(-kw["cout"] // 32) * 32}), 0
    if op == "wide":
        cp = -(-cin // 32) * 32
        return "split16", CC.conv_args(cin_pad=cp, lda=cp, x=CC.SPLIT, w=CC.SPLIT, **{**kw, "ldo": -(-kw["cout"] // 32) * 32}), 0
    a = CC.conv_args(**kw)
    if op == "seg":
        return "seg_gemm", a, int(lib.sd_seg_gemm_scratch_bytes(a.M, a.cin_pad, a.cout))
    return op, a, 0


def set_tuning(N, sel, tune):
    from kernel_selection import select_conv_kernel
    select_conv_kernel(sel)
    N.check(N.load().sd_set_tuning(N.SD_TUNE_F16_NARROW_TILES, tune.get("f16_tiles", -1)), "sd_set_tuning")
    N.check(N.load().sd_set_tuning(N.SD_TUNE_T256_LOCKSTEP_TILES, tune.get("lockstep", -1)), "sd_set_tuning")


def read(a):
    from speech_diarization_amd import _native as N
    lib = N.load()
    rec = {}
    for key, op, kw, sel, tune in shape_list():
        set_tuning(N, sel, tune)
        entry, args, scratch = build_args(op, kw, lib)
        rec[key] = sorted(ln[0] for ln in N.conv_choice_read(args, entry, a.n_cu, scratch))
    set_tuning(N, "auto", {})
    return rec


def launch(a):
    """Every shape through its public entry.  One zero-filled buffer per kind of operand (x, w, y, vectors, tee, scratch, colstat), sized
    for the largest extent of that kind over the whole list before anything is launched; each pointer of the arguments is replaced
    by that buffer's."""
    import torch
    import launch_log as L
    from forward_census import bind_what_the_library_has
    N = bind_what_the_library_has()
    lib = N.load()
    dev = torch.device("cuda", 0)
    shapes = [(key, sel, tune) + build_args(op, kw, lib) + (op,) for key, op, kw, sel, tune in shape_list()]
    need = collections.Counter()
    for _, _, _, entry, p, scratch, _ in shapes:
        esz = lambda dt: 2 if dt == N.SD_DT_F16 else 4  # noqa: E731
        for buf, n in (("x", p.M * p.lda * esz(p.x_dtype)), ("w", p.cout * p.taps * p.cin_pad * esz(p.w_dtype)), ("y", p.M * p.ldo * esz(p.y_dtype)),
                       ("vec", p.M * p.cout * 4 if p.bias_per_seg else p.cout * 4), ("tee", p.M * max(p.ldt, p.ld_ta) * 4), ("scratch", scratch),
                       ("colstat", int(lib.sd_colstat_floats(p.M, p.cout)) * 4 if p.colstat else 0)):
            need[buf] = max(need[buf], n)
    mem = {k: torch.zeros(max(n, 16), dtype=torch.uint8, device=dev) for k, n in need.items()}
    spans = {}
    rec = {}
    entries = {"f32": lib.sd_conv1d_cl_f32, "f16": lib.sd_conv1d_cl_f16, "split16": lib.sd_conv1d_cl_split16}
    for key, sel, tune, entry, p, scratch, op in shapes:
        set_tuning(N, sel, tune)
        p.x, p.w, p.y = mem["x"].data_ptr(), mem["w"].data_ptr(), mem["y"].data_ptr()
        p.bias = p.scale = p.shift = mem["vec"].data_ptr()
        if p.tee:
            p.tee = mem["tee"].data_ptr()
        if p.tee_add:
            p.tee_add = mem["tee"].data_ptr()
        if p.colstat:
            p.colstat = mem["colstat"].data_ptr()
        with L.launches() as log:
            if entry == "packed":
                B = p.M // T if p.M % T == 0 and p.M >= T else 5
                if (p.M, B) not in spans:
                    spans[p.M, B] = torch.linspace(0, p.M, B + 1, device=dev).to(torch.int32)
                N.check(lib.sd_conv1d_cl_packed_f32(C.byref(p), spans[p.M, B].data_ptr(), B, None), key)
            elif entry == "seg_gemm":
                N.check(lib.sd_seg_gemm_f32(C.byref(p), mem["scratch"].data_ptr() if scratch else None, scratch, None), key)
            else:
                N.check(entries[entry](C.byref(p), None), key)
        torch.cuda.synchronize()
        rec[key] = sorted(lb for lb, n in log.items() for _ in range(n))
    set_tuning(N, "auto", {})
    return rec


def diff(a):
    old, new = (json.load(open(p)) for p in a.diff)
    keys = sorted(set(old["labels"]) | set(new["labels"]))
    differing = [k for k in keys if old["labels"].get(k) != new["labels"].get(k)]
    per_op = collections.Counter(k.split("/")[1] for k in keys)
    rec = {"launched": {"library": old["library"], "how": old["how"]}, "read": {"library": new["library"], "how": new["how"], "n_cu": new.get("n_cu")},
           "summary": {"shapes": len(keys), "per_operator": dict(per_op), "identical": len(keys) - len(differing), "differing": differing},
           "labels": old["labels"]}
    rec["launched"]["commit"] = a.parent_commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    if a.forwards:      # the summary of `tools/forward_census.py --diff` for the same two libraries
        rec["forward_census"] = json.load(open(a.forwards))["summary"]
    if a.bench:
        runs = json.load(open(a.bench))
        rec["bench"] = {"runs": runs}
        for metric in ("value", "numpy_batch32"):
            by = {lib: [r[metric] for r in runs if r["library"] == lib] for lib in ("parent", "new")}
            spread = max(by["parent"]) - min(by["parent"])
            gap = abs(statistics.median(by["new"]) - statistics.median(by["parent"]))
            rec["bench"][metric] = {"parent_median": statistics.median(by["parent"]), "new_median": statistics.median(by["new"]), "parent_spread": spread,
                                    "within_parent_spread": gap <= spread}
    with open(a.summary, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for k in differing:
        print("DIFFERS", k, old["labels"].get(k), new["labels"].get(k))
    print(f"{len(keys) - len(differing)} shapes identical, {len(differing)} differ -> {a.summary}")
    return 1 if differing or not keys else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launch", action="store_true")
    ap.add_argument("--read", action="store_true")
    ap.add_argument("--n-cu", type=int, default=256)
    ap.add_argument("--out")
    ap.add_argument("--diff", nargs=2, metavar=("LAUNCHED", "READ"))
    ap.add_argument("--bench", help="JSON list of the alternated bench.py runs")
    ap.add_argument("--forwards", help="the summary file of `tools/forward_census.py --diff` for the same two libraries")
    ap.add_argument("--parent-commit", default=None, help="the commit of the LAUNCHED record (default: HEAD, for an uncommitted change)")
    ap.add_argument("--summary", default=os.path.join(ROOT, "profiles", "conv_choice_parity.json"))
    a = ap.parse_args()
    if a.diff:
        sys.exit(diff(a))
    labels = launch(a) if a.launch else read(a)
    variant = os.environ.get("SD_HIP_LIB") if os.environ.get("SD_EXPERIMENT") == "1" else None
    rec = {"library": os.path.relpath(os.path.abspath(variant or os.path.join(ROOT, "speech-diarization_amd", "libsd_hip.so")), ROOT),
           "how": "launch log" if a.launch else "sd_conv_choice_read", "labels": labels}
    if a.read:
        rec["n_cu"] = a.n_cu
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    per_op = collections.Counter(k.split("/")[1] for k in labels)
    print(f"{len(labels)} shapes ({dict(per_op)}) -> {a.out}")
