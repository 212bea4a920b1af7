#!/usr/bin/env python3
"""Two builds of libsd_hip.so refuse the same calls of the eight entries that take f32 rows, with the same status code and the same
sd_last_error text (build container: no GPU is touched, and none is needed).

    python tools/rows_check_parity.py --parent speech-diarization_amd/variants/libsd_hip_parent.so [--out FILE]
    python tools/rows_check_parity.py --record FILE          one library, one process (the other one: SD_EXPERIMENT=1 SD_HIP_LIB=...)

The calls are the table of tests/helpers/rows_cases.py: every rule of every entry alone and every pair of rules adjacent in an entry's
order broken together, on invented non-null pointers.  The table holds refusals only, because a call that passed every check would
launch on those pointers: `--parent` records the parent's library first, in a process of its own, and stops unless it refused every
row with an argument, support or workspace code; only then is this checkout's library asked.  The record of both, row by row, goes to
profiles/rows_check_parity.json; exit status 1 if a row differs."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))


def record(path):
    import rows_cases as R

    from speech_diarization_amd import _native as N
    lib = N.load()
    rows = []
    for entry, args, _, _ in R.REFUSALS:
        status = int(R.call_library(lib, entry, args))
        rows.append({"entry": R.NAME[entry], "call": R.pure_spec(entry, args), "status": status, "text": N.last_error()})
        if status not in (R.ARG, R.UNSUP, R.WS):
            sys.exit(f"not refused: {rows[-1]}")
    with open(path, "w") as fh:
        json.dump({"library": os.path.basename(os.environ.get("SD_HIP_LIB") or str(N.LIB_PATH)), "rows": rows}, fh, indent=1)
    print(f"{len(rows)} calls, all refused -> {path}")


def both(parent, out):
    import rows_cases as R
    records = []
    tmp = tempfile.TemporaryDirectory(prefix="rows_check_parity_")
    for name, env in (("parent", {"SD_EXPERIMENT": "1", "SD_HIP_LIB": os.path.abspath(parent)}), ("new", {})):
        path = os.path.join(tmp.name, name + ".json")
        clean = {k: v for k, v in os.environ.items() if k not in ("SD_EXPERIMENT", "SD_HIP_LIB")}
        ran = subprocess.run([sys.executable, os.path.abspath(__file__), "--record", path], env={**clean, **env})
        if ran.returncode != 0:
            sys.exit(f"the {name} library did not refuse every row: nothing further is run")
        records.append(json.load(open(path)))
    tmp.cleanup()
    a, b = records
    differ = [(x, y) for x, y in zip(a["rows"], b["rows"]) if x != y]
    expected = [{"status": code, "text": text} for _, _, code, text in R.REFUSALS]
    off_table = [x for x, w in zip(b["rows"], expected) if (x["status"], x["text"]) != (w["status"], w["text"])]
    equal = len(a["rows"]) == len(b["rows"]) == len(R.REFUSALS) and not differ
    result = {"parent": a["library"], "new": b["library"], "calls": len(a["rows"]), "entries": sorted({r["entry"] for r in a["rows"]}),
              "equal": equal, "differ": differ, "differ_from_the_written_table": off_table, "rows": a["rows"]}
    with open(out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: result[k] for k in ("parent", "new", "calls", "equal")}), f"{len(differ)} differ, {len(off_table)} differ from the written table")
    for x, y in differ[:10]:
        print("  ", x, "\n  ", y)
    return 0 if equal and not off_table else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--record")
    ap.add_argument("--parent")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rows_check_parity.json"))
    args = ap.parse_args()
    if args.record:
        record(args.record)
    if args.parent:
        sys.exit(both(args.parent, args.out))
