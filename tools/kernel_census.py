#!/usr/bin/env python3
"""Merge the launch census of the GPU suite -> profiles/kernel_census.json (a record; no test reads it).

Taking the census is a job of its own on the MI355X and nothing in the repository starts it: run every tests/test_gpu_*.py in a
process of its own, each under a time limit of its own and chained so that ANY non-zero exit status (a failed test may be a faulted
device) ends the job, with

    SD_EXPERIMENT=1 SD_LAUNCH_LOG=<dir>/<module>.tsv python -m pytest tests/<module>.py -q -m gpu

so that the library counts every launch of that process and writes "label<TAB>count" lines at exit (include/sd_hip_trace.h).  Then

    python tools/kernel_census.py <dir>

merges the files: label -> launches per module, the commit, and the labels of csrc/*.hip (the regex of
tests/test_launch_log_rules.py) that no module reached, which must equal tests/helpers/kernel_census.EXEMPT."""
import argparse
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = re.compile(r'"([a-z0-9_]+_kernel(?:<[^">]*>)?(?:/[a-z]+)?)"')


def source_labels():
    out = set()
    for f in glob.glob(os.path.join(ROOT, "speech-diarization_amd", "csrc", "*.hip")):
        out |= set(LABEL.findall(open(f).read()))
    return out


def merge(out_dir, commit):
    labels = {}
    modules = []
    for f in sorted(glob.glob(os.path.join(out_dir, "test_gpu_*.tsv"))):
        module = os.path.basename(f)[:-4]
        modules.append(module)
        for line in open(f).read().splitlines():
            label, _, count = line.rpartition("\t")
            labels.setdefault(label, {})[module] = int(count)
    known = source_labels()
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import kernel_census
    rec = {"commit": commit, "device": "MI355X (256 CUs), shipped tuning defaults", "modules": modules,
           "launches": {lb: labels[lb] for lb in sorted(labels)},
           "unreached": sorted(known - set(labels)), "exempt": sorted(kernel_census.EXEMPT),
           "not_in_sources": sorted(set(labels) - known)}
    with open(os.path.join(ROOT, "profiles", "kernel_census.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(f"{len(labels)} labels over {len(modules)} modules; unreached: {rec['unreached']}")
    return rec["unreached"] == rec["exempt"] and not rec["not_in_sources"]


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("dir", help="the folder of <module>.tsv files")
    ap.add_argument("--commit", default=None, help="the commit the census was taken on (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    sys.exit(0 if merge(a.dir, commit) else 1)
