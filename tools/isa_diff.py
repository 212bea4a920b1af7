#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel (build container: hipcc cross-compiles, no GPU).

    python tools/isa_diff.py [TREE_A [TREE_B]] [--rev REV] [--files a.hip,b.hip] [--out FILE] [--show SUBSTR]

TREE_A defaults to this checkout; TREE_B defaults to a `git archive` of REV under a temporary folder, and REV to the parent of what
TREE_A holds: HEAD while csrc/ or include/ carry uncommitted changes, HEAD~1 once they are committed.  Every file of each tree's
own build_native.SOURCES is compiled with build_native's flags plus `--offload-device-only -S` (at most 16 compiles at a time), the
assembly is cut into functions at their symbol labels, comments, `.ident` and `.file` are dropped, the function's position in the
file is taken out of its local labels (.LBB<n>_<block> -> .LBB_<block>: the order in which templates are instantiated follows the host
code), and each function's text is compared as text: nothing here looks for a particular instruction.  Per kernel: identical or not, the number of differing lines
(`diff`), and from the metadata block of either side vgpr_count, agpr_count, sgpr_count, private_segment_fixed_size, vgpr_spill_count
and group_segment_fixed_size.  What lies outside every function (device variables, the target line) is compared as one more entry
per file.  The record goes to profiles/isa_diff_conv_shared.json (--out) with the commit of each side and the `hipcc --version`
line.  Exit status: 1 if a kernel or a source file exists on one side only or a compile fails, else 0 (differences are reported,
not judged: which kernels may differ is the reader's rule)."""
import argparse
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "speech-diarization_amd"
RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size")
BEGIN = re.compile(r"^\t\.(?:globl|weak|protected|hidden)\t(\S+)\s*; -- Begin function ")
ORDINAL = re.compile(r"(\.L(?:BB|JTI|func_begin|func_end))\d+")     # .LBB<n>_<block>: n is the function's position in the file
TAIL = re.compile(r"^\t\.(?:section\t\.AMDGPU\.gpr_maximums|amdgpu_metadata)")


def load_build_native(tree):
    spec = importlib.util.spec_from_file_location("build_native_" + str(abs(hash(tree))), os.path.join(tree, PKG, "build_native.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def git(tree, *args):
    r = subprocess.run(["git", "-C", tree] + list(args), capture_output=True, text=True)
    return r.stdout.strip() if r.returncode == 0 else None


def describe(tree):
    commit = git(tree, "rev-parse", "HEAD")
    dirty = bool(git(tree, "status", "--porcelain", "--", PKG + "/csrc", "include")) if commit else None
    return {"dir": os.path.relpath(tree, ROOT), "commit": commit, "uncommitted_source_changes": dirty}


def compile_tree(tree, flags, sources, out_dir, pool):
    os.makedirs(out_dir, exist_ok=True)
    inc = [f"-I{os.path.join(tree, 'include')}", f"-I{os.path.join(tree, PKG, 'csrc')}"]

    def one(src):
        out = os.path.join(out_dir, src + ".s")
        os.makedirs(os.path.dirname(out), exist_ok=True)      # (a source in a subdirectory: diag/, ahc/)
        cmd = flags + inc + ["--offload-device-only", "-S", os.path.join(tree, PKG, "csrc", src), "-o", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.stderr.write(f"--- {tree}: {src}\n{r.stdout}\n")
            return src, None
        return src, out
    return [pool.submit(one, s) for s in sources]


def strip(lines):
    out = []
    for ln in lines:
        s = ln.lstrip()
        if not s or s.startswith(";") or s.startswith("//") or s.startswith(".ident") or s.startswith(".file"):
            continue
        if ";" in ln and '"' not in ln:
            ln = ln.split(";")[0]                 # a trailing comment (it may name a block of the function by its ordinal)
        out.append(ORDINAL.sub(r"\1", ln.rstrip()))
    return out


def cut(path):
    """-> ({symbol: stripped lines}, stripped lines outside every function, {symbol: metadata fields} of the kernels)"""
    lines = open(path).read().split("\n")
    starts = []
    for i, ln in enumerate(lines):
        m = BEGIN.match(ln)
        if m:
            starts.append((i - 1 if i and re.match(r"^\t\.(?:section\t\.text|text)", lines[i - 1]) else i, m.group(1)))
    end = len(lines)
    if starts:
        for i in range(starts[-1][0], len(lines)):
            if TAIL.match(lines[i]):
                end = i
                break
    funcs = {}
    for k, (i, sym) in enumerate(starts):
        j = starts[k + 1][0] if k + 1 < len(starts) else end
        funcs[sym] = strip(lines[i:j])
    other = lines[:starts[0][0]] if starts else []
    # the metadata block: one entry per kernel, compared (and reported) with its kernel, not with the rest of the file
    meta, entries, cur, in_kernels = {}, [], None, False
    for ln in lines[end:]:
        if ln.startswith("amdhsa.kernels:"):
            in_kernels = True
        elif in_kernels and ln.startswith("amdhsa."):
            in_kernels = False
        elif in_kernels and ln.startswith("  - "):
            cur = {"text": [ln]}
            entries.append(cur)
            ln = "    " + ln[4:]
        elif in_kernels and cur is not None:
            cur["text"].append(ln)
        else:
            other.append(ln)
            continue
        m = re.match(r"^    (\.[a-z_]+):\s+(\S+)$", ln)
        if m and cur is not None and in_kernels:
            cur[m.group(1)[1:]] = m.group(2)
    for e in entries:
        meta[e["name"]] = e
        funcs[e["name"]] = funcs.get(e["name"], []) + strip(e.pop("text"))
    other = [ln for ln in strip(other) if "__hip_cuid_" not in ln]      # a per-compilation id, not device code
    return funcs, other, meta


def n_diff_lines(a, b, tmp):
    pa, pb = os.path.join(tmp, "a.txt"), os.path.join(tmp, "b.txt")
    for p, t in ((pa, a), (pb, b)):
        with open(p, "w") as f:
            f.write("\n".join(t) + "\n")
    r = subprocess.run(["diff", pa, pb], capture_output=True, text=True)
    return sum(1 for ln in r.stdout.split("\n") if ln[:1] in "<>" and ln), r.stdout


def demangle(symbols):
    exe = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not exe or not symbols:
        return {s: s for s in symbols}
    r = subprocess.run([exe], input="\n".join(symbols) + "\n", capture_output=True, text=True)
    names = r.stdout.split("\n")[:len(symbols)]
    return {s: n.replace("(anonymous namespace)::", "") for s, n in zip(symbols, names)} if len(names) == len(symbols) else {s: s for s in symbols}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a", nargs="?", default=ROOT)
    ap.add_argument("tree_b", nargs="?", default=None)
    ap.add_argument("--rev", default=None, help="the commit archived as TREE_B when no directory is given")
    ap.add_argument("--files", default=None, help="comma-separated subset of build_native.SOURCES")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isa_diff_conv_shared.json"))
    ap.add_argument("--show", default=None, help="print the diff of every differing function whose name contains this")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    tree_a = os.path.abspath(a.tree_a)
    tmp = tempfile.mkdtemp(prefix="isa_diff_")
    try:
        side_a = describe(tree_a)
        if a.tree_b:
            tree_b = os.path.abspath(a.tree_b)
            side_b = describe(tree_b)
        else:
            rev = a.rev or ("HEAD" if side_a["uncommitted_source_changes"] else "HEAD~1")
            tree_b = os.path.join(tmp, "tree_b")
            os.makedirs(tree_b)
            ar = subprocess.run(["git", "-C", tree_a, "archive", rev, PKG, "include"], capture_output=True)
            if ar.returncode != 0:
                sys.exit(f"git archive {rev} failed: {ar.stderr.decode()}")
            subprocess.run(["tar", "-x", "-C", tree_b], input=ar.stdout, check=True)
            side_b = {"dir": f"git archive {rev}", "commit": git(tree_a, "rev-parse", rev), "uncommitted_source_changes": False}
        bn_a, bn_b = load_build_native(tree_a), load_build_native(tree_b)
        flags = load_build_native(ROOT).compile_flags()[:]
        flags = [f for f in flags if not f.startswith("-I")]
        src_a, src_b = list(bn_a.SOURCES), list(bn_b.SOURCES)
        if a.files:
            want = a.files.split(",")
            src_a, src_b = [s for s in src_a if s in want], [s for s in src_b if s in want]
        version = subprocess.run([flags[0], "--version"], capture_output=True, text=True).stdout.split("\n")
        version = next((ln for ln in version if "clang version" in ln), version[0])
        with ThreadPoolExecutor(max(1, min(16, a.jobs))) as pool:
            fa = compile_tree(tree_a, flags, src_a, os.path.join(tmp, "a"), pool)
            fb = compile_tree(tree_b, flags, src_b, os.path.join(tmp, "b"), pool)
            asm_a, asm_b = dict(f.result() for f in fa), dict(f.result() for f in fb)
        failed = [s for s, p in list(asm_a.items()) + list(asm_b.items()) if p is None]
        one_sided = sorted(set(src_a) ^ set(src_b))
        rows = []
        for src in [s for s in src_a if s in asm_b and asm_a[s] and asm_b[s]]:
            fa_, oa, ma = cut(asm_a[src])
            fb_, ob, mb = cut(asm_b[src])
            names = demangle(sorted(set(fa_) | set(fb_)))
            for sym in sorted(set(fa_) | set(fb_), key=lambda s: names[s]):
                row = {"file": src, "name": names[sym], "symbol": sym, "kernel": sym in ma or sym in mb}
                if sym not in fa_ or sym not in fb_:
                    row["only_in"] = "a" if sym in fa_ else "b"
                    one_sided.append(f"{src}: {names[sym]}")
                else:
                    row["identical"] = fa_[sym] == fb_[sym]
                    row["lines"] = len(fa_[sym])
                    if not row["identical"]:
                        row["differing_lines"], text = n_diff_lines(fa_[sym], fb_[sym], tmp)
                        if a.show and a.show in names[sym]:
                            print(f"=== {names[sym]}\n{text}")
                for side, m in (("a", ma), ("b", mb)):
                    if sym in m:
                        row[side] = {k: int(m[sym][k]) for k in RESOURCES if k in m[sym]}
                rows.append(row)
            row = {"file": src, "name": "(outside every function)", "kernel": False, "identical": oa == ob, "lines": len(oa)}
            if oa != ob:
                row["differing_lines"], text = n_diff_lines(oa, ob, tmp)
                if a.show is not None and a.show in row["name"]:
                    print(f"=== {src} {row['name']}\n{text}")
            rows.append(row)
        both = [r for r in rows if "identical" in r]
        differing = [r for r in both if not r["identical"]]
        rec = {"hipcc_version": version, "flags": flags[1:] + ["--offload-device-only", "-S"], "a": side_a, "b": side_b,
               "summary": {"functions": len(both), "kernels": sum(r["kernel"] for r in both), "identical": len(both) - len(differing),
                           "differing": [f"{r['file']}: {r['name']}" for r in differing], "one_side_only": one_sided,
                           "compile_failed": failed},
               "functions": rows}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        for r in differing:
            ra, rb = r.get("a", {}), r.get("b", {})
            res = " ".join(f"{k.replace('_count', '').replace('_fixed_size', '')} {ra.get(k)}/{rb.get(k)}" for k in RESOURCES if k in ra or k in rb)
            print(f"DIFFERS {r['file']}: {r['name']}: {r['differing_lines']} lines; a/b: {res}")
        for s in one_sided:
            print(f"ONE SIDE ONLY {s}")
        for s in failed:
            print(f"COMPILE FAILED {s}")
        print(f"{len(both)} functions ({rec['summary']['kernels']} kernels) on both sides: {len(both) - len(differing)} identical, {len(differing)} differ"
              f" -> {os.path.relpath(a.out, ROOT)}")
        return 1 if one_sided or failed else 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
