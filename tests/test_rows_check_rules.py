"""No-GPU checks of the check of the eight entries that take f32 rows (csrc/sd_rows_check.h): what such an entry
refuses, with which status code, text and precedence, and how many bytes its workspace has, is a pure function of a description of the
call, so it is checked here at the integer limits and not only where a caller happens to pass.

tests/helpers/rows_check_pure.cpp is the header alone in a plain C++ program with its own main, built here with the address and
undefined-behaviour sanitizers (nothing preloaded).  The refusals are the hand-written table of tests/helpers/rows_cases.py; the sizes
are derived by hand from the kernels' geometry (128-row tiles, T + 1 or 2 W + 2 argmax slots of 8 bytes per padded row, eight column
tiles per workgroup of the core pass, 512-row blocks of 16 T + 256 T (T + 1) / 2 doubles), not read off the code under test."""
import os
import re
import shutil
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import rows_cases as R  # noqa: E402
from rows_cases import ARG, UNSUP, WS  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402

CSRC = N.PKG_DIR / "csrc"
INT_MAX, INT_MIN, LONG_MAX, LONG_MIN = 2**31 - 1, -2**31, 2**63 - 1, -2**63
FILES = ("sd_ahc.hip", "ahc/sd_ahc_grouped.hip", "sd_hdbscan.hip", "diag/sd_diag.hip")


@pytest.fixture(scope="module")
def pure(tmp_path_factory):
    cxx = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert os.path.exists(cxx), "no clang++ on this machine"
    exe = tmp_path_factory.mktemp("rows_check") / "rows_check_pure"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{CSRC}",
           f"-I{N.PKG_DIR.parent / 'include'}", os.path.join(HERE, "helpers", "rows_check_pure.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr

    def run(*calls):
        ran = subprocess.run([str(exe), *calls], capture_output=True, text=True)
        assert ran.returncode == 0 and not ran.stderr, (ran.returncode, ran.stderr[-2000:])
        return ran.stdout.splitlines()
    return run


def parse(line):
    if " why=" in line:
        status, why = line.split(" why=", 1)
        return int(status.split("=")[1]), why
    status, need = line.split()
    return int(status.split("=")[1]), int(need.split("=")[1])


def ask(pure, entry, **args):
    (line,) = pure(R.pure_spec(entry, args))
    return parse(line)


# ------------------------------------------------------------------ refusals: code, full text, precedence

def test_the_table_covers_every_rule_of_every_entry():
    """The rules an entry has, counted from its description: the shape message, the limit on d (not sd_ahc_merge_f32), its own rules, the
    null pointer, the rows' alignment, and with a workspace its alignment, the grid limit (not the statistics) and its size."""
    rules = {"nearest": 7, "outgoing": 7, "merge": 3, "grouped": 8, "core": 9, "stats": 6, "apply": 4, "centroids": 5}
    for entry, count in rules.items():
        texts = {re.sub(r"-?\d+", "#", text) for e, _, _, text in R.REFUSALS if e == entry}
        texts = {t.split(" (ld=")[0] for t in texts}                  # (one rule whatever the ld it quotes)
        texts = {"shape" if re.search(r": n=# d=#( k=#)? ld=#", t) else t for t in texts}
        assert len(texts) == count, (entry, sorted(texts))
    assert {code for _, _, code, _ in R.REFUSALS} == {ARG, UNSUP, WS}
    assert all(text.startswith(R.NAME[e] + ": ") for e, _, _, text in R.REFUSALS)


def test_every_refusal_has_its_code_its_text_and_its_precedence(pure):
    got = [parse(line) for line in pure(*(R.pure_spec(e, a) for e, a, _, _ in R.REFUSALS))]
    assert len(got) == len(R.REFUSALS) == 153
    for (entry, args, code, text), g in zip(R.REFUSALS, got):
        assert g == (code, text), (entry, args, g)


def test_the_entries_are_wired_to_the_check():
    """The same table through the built library: every entry describes itself as rows_check_pure.cpp describes it."""
    lib = N.load()
    for entry, args, code, text in R.REFUSALS:
        status = R.call_library(lib, entry, args)
        assert (status, N.last_error()) == (code, text), (entry, args)


def test_calls_on_the_accepted_side_of_every_rule_pass(pure):
    assert ask(pure, "nearest") == (0, 2048) and ask(pure, "outgoing", n=65535 * 128) == (0, 65536 * 65535 * 1024)
    assert ask(pure, "nearest", d=1024, ld=1024) == (0, 2048) and ask(pure, "nearest", d=1, ld=4) == (0, 2048)
    assert ask(pure, "nearest", ws=2048)[0] == 0 and ask(pure, "nearest", ws=2**62)[0] == 0
    assert ask(pure, "merge", d=5000, ld=5000) == (0, 0)                       # no limit on d: one thread walks a row
    assert ask(pure, "merge", flags="m", ws=0) == (0, 0)                       # and no workspace to look at
    assert ask(pure, "apply", flags="m", ws=0) == (0, 0) and ask(pure, "centroids", flags="m", ws=0, k=1024) == (0, 0)
    assert ask(pure, "grouped", k=1) == (0, 2048) and ask(pure, "grouped", n=R.BIG_N, k=65534 * 128 + 1) == (0, 131070 * 65536 * 1024)
    assert ask(pure, "grouped", n=R.BIG_N, k=1) == (0, 2 * 65536 * 1024)      # no limit on the rows of a band
    assert ask(pure, "core", k=16) == (0, 8192) and ask(pure, "core", n=17, k=16) == (0, 8192) and ask(pure, "core", n=2, k=1) == (0, 512)
    assert ask(pure, "stats", n=2, d=256, ld=256, ld2=256) == (0, 280576) and ask(pure, "stats", n=2**30, d=1, ld=4)[0] == 0


# ------------------------------------------------------------------ the five workspace sizes, by hand

SIZES = [
    # (T + 1) T slots of 128 rows, 8 bytes each
    ("nearest", 1, 192, 0, 2048), ("nearest", 127, 192, 0, 2048), ("nearest", 128, 192, 0, 2048), ("nearest", 129, 192, 0, 6144),
    ("nearest", 65535 * 128, 1, 0, 65536 * 65535 * 1024), ("nearest", 65535 * 128 + 1, 1024, 0, 65537 * 65536 * 1024),
    ("outgoing", 1, 7, 0, 2048), ("outgoing", 127, 7, 0, 2048), ("outgoing", 128, 7, 0, 2048), ("outgoing", 129, 7, 0, 6144),
    ("outgoing", 65535 * 128, 192, 0, 65536 * 65535 * 1024),
    # (2 W + 2) T slots, W = min(T - 1, ceil((max_group - 1) / 128))
    ("grouped", 1, 192, 1, 2048), ("grouped", 127, 192, 127, 2048), ("grouped", 128, 192, 128, 2048), ("grouped", 129, 192, 1, 4096),
    ("grouped", 129, 192, 2, 8192), ("grouped", 129, 192, 129, 8192), ("grouped", 1000, 192, INT_MAX, 16 * 8 * 1024),
    ("grouped", 65535 * 128 + 1, 192, 65534 * 128 + 1, 131070 * 65536 * 1024), ("grouped", 65535 * 128 + 1, 192, 65534 * 128 + 2, 131072 * 65536 * 1024),
    # ceil(T / 8) T slots of 128 rows, k floats each; k <= n - 1
    ("core", 1, 192, 1, 0), ("core", 127, 192, 1, 512), ("core", 128, 192, 2, 1024), ("core", 129, 192, 2, 2048), ("core", 129, 192, 16, 16384),
    ("core", 1025, 192, 2, 2 * 9 * 128 * 2 * 4), ("core", 65535 * 128, 192, 16, 8192 * 65535 * 128 * 16 * 4),
    # ceil(n / 512) blocks of 16 T + 256 T (T + 1) / 2 doubles, T = ceil(d / 16); n >= 2
    ("stats", 1, 192, 0, 0), ("stats", 127, 192, 0, 161280), ("stats", 128, 192, 0, 161280), ("stats", 129, 192, 0, 161280),
    ("stats", 2, 1, 0, 2176), ("stats", 513, 17, 0, 12800), ("stats", 2, 256, 0, 280576),
    # the integer limits
    ("nearest", INT_MAX, 1, 0, (2**24 + 1) * 2**24 * 1024), ("grouped", INT_MAX, 1, INT_MAX, 2**59), ("grouped", INT_MAX, 1, 1, 2**35),
    ("core", INT_MAX, 192, 16, 2**21 * 2**24 * 128 * 16 * 4), ("stats", INT_MAX, 256, 0, 2**22 * 280576),
    # outside the supported range: 0
    ("nearest", 0, 192, 0, 0), ("nearest", INT_MIN, 192, 0, 0), ("nearest", 100, 0, 0, 0), ("nearest", 100, 1025, 0, 0), ("nearest", 100, INT_MAX, 0, 0),
    ("grouped", 100, 192, 0, 0), ("grouped", 100, 192, INT_MIN, 0), ("grouped", 100, 1025, 5, 0), ("core", 100, 192, 0, 0), ("core", 100, 192, 17, 0),
    ("core", 100, 192, INT_MAX, 0), ("core", 10, 192, 10, 0), ("core", INT_MIN, 192, 1, 0), ("stats", 100, 257, 0, 0), ("stats", INT_MIN, 192, 0, 0),
]


def test_the_workspace_sizes_equal_the_hand_derived_values(pure):
    got = pure(*(f"size:{e}:{n}:{d}:{k}" for e, n, d, k, _ in SIZES))
    assert [int(x) for x in got] == [want for *_, want in SIZES]
    # an entry without a workspace has no size
    assert [int(x) for x in pure("size:merge:100:192:0", "size:apply:100:192:0", "size:centroids:100:192:4")] == [0, 0, 0]


def test_the_size_functions_of_the_library_are_the_headers():
    lib = N.load()
    fn = {"nearest": lib.sd_ahc_nearest_workspace_bytes, "outgoing": lib.sd_hdb_outgoing_workspace_bytes, "stats": lib.sd_whiten_stats_workspace_bytes,
          "grouped": lib.sd_ahc_nearest_grouped_workspace_bytes, "core": lib.sd_hdb_core_workspace_bytes}
    for e, n, d, k, want in SIZES:
        assert int(fn[e](n, d, k) if e in ("grouped", "core") else fn[e](n, d)) == want, (e, n, d, k)


# ------------------------------------------------------------------ the integer limits, under the sanitizers

def test_the_integer_limits(pure):
    rows = "n=2147483647, at most 8388480 rows are supported"
    for entry, name in (("nearest", "sd_ahc_nearest_f32"), ("outgoing", "sd_hdb_outgoing_f32"), ("core", "sd_hdb_core_f32")):
        assert ask(pure, entry, n=INT_MAX, k=16) == (UNSUP, f"{name}: {rows}")
        assert ask(pure, entry, n=INT_MAX, k=16, ws=0) == (UNSUP, f"{name}: {rows}")
        assert ask(pure, entry, n=INT_MIN, k=1) == (ARG, f"{name}: n=-2147483648 d=192 ld=192")
        assert ask(pure, entry, d=INT_MAX, ld=LONG_MAX, k=1) == (UNSUP, f"{name}: d=2147483647, at most 1024 columns are supported")
        assert ask(pure, entry, d=INT_MIN, ld=LONG_MIN, k=1) == (ARG, f"{name}: n=100 d=-2147483648 ld=-9223372036854775808")
        assert ask(pure, entry, ld=LONG_MAX, k=1)[1].endswith("with ld % 4 == 0 (ld=9223372036854775807)")
        assert ask(pure, entry, ld=LONG_MAX - 3, k=1)[0] == 0
        assert ask(pure, entry, ws=2**63 - 1, k=1)[0] == 0
    g = "sd_ahc_nearest_grouped_f32"
    assert ask(pure, "grouped", n=INT_MAX, k=INT_MAX) == (UNSUP, f"{g}: max_group=2147483647, a group of at most 8388352 rows is supported")
    assert ask(pure, "grouped", n=INT_MAX, k=1) == (0, 2**35)
    assert ask(pure, "grouped", n=INT_MAX, k=1, ws=0) == (WS, f"{g}: workspace of 0 bytes, n=2147483647 d=192 max_group=1 needs 34359738368")
    assert ask(pure, "grouped", n=100, k=INT_MAX) == (0, 2048) and ask(pure, "grouped", k=INT_MIN) == (ARG, f"{g}: max_group=-2147483648")
    assert ask(pure, "core", k=INT_MAX) == (UNSUP, "sd_hdb_core_f32: k=2147483647, at most 16 neighbours are supported")
    assert ask(pure, "core", k=INT_MIN) == (ARG, "sd_hdb_core_f32: k=-2147483648 must lie in 1 .. n - 1 (n=100)")
    assert ask(pure, "core", n=INT_MAX, k=16, ws=2**63 - 1)[0] == UNSUP
    assert ask(pure, "merge", n=INT_MAX, d=INT_MAX, ld=LONG_MAX - 3) == (0, 0)
    assert ask(pure, "merge", n=INT_MAX, d=INT_MAX, ld=INT_MAX - 1) == (ARG, "sd_ahc_merge_f32: n=2147483647 d=2147483647 ld=2147483646")
    s = "sd_whiten_stats_f64"
    assert ask(pure, "stats", n=INT_MAX, d=256, ld=256, ld2=256) == (0, 2**22 * 280576)
    assert ask(pure, "stats", n=INT_MAX, d=256, ld=256, ld2=256, ws=0) == (WS, f"{s}: workspace of 0 bytes, n=2147483647 d=256 needs 1176821039104")
    assert ask(pure, "stats", n=INT_MIN, d=INT_MIN, ld=LONG_MIN, ld2=LONG_MIN) == (
        ARG, f"{s}: n=-2147483648 d=-2147483648 ld=-9223372036854775808 ldg=-9223372036854775808 (n >= 2: one row has no covariance)")
    assert ask(pure, "stats", ld2=LONG_MAX)[0] == 0
    assert ask(pure, "apply", n=INT_MAX, ld2=LONG_MAX, ld3=LONG_MAX) == (0, 0)
    assert ask(pure, "apply", n=INT_MIN, ld2=LONG_MIN, ld3=LONG_MAX) == (
        ARG, "sd_whiten_apply_f64: n=-2147483648 d=192 ld=192 ldw=-9223372036854775808 ldo=9223372036854775807")
    c = "sd_label_centroids_f32"
    assert ask(pure, "centroids", n=INT_MAX, k=1024, ld2=LONG_MAX) == (0, 0)
    assert ask(pure, "centroids", k=INT_MAX) == (UNSUP, f"{c}: k=2147483647, at most 1024 labels are supported")
    assert ask(pure, "centroids", k=INT_MIN, ld2=LONG_MIN) == (ARG, f"{c}: n=100 d=192 k=-2147483648 ld=192 ldo=-9223372036854775808")


# ------------------------------------------------------------------ one statement of the contract

def _code(text):
    return re.sub(r"//[^\n]*", "", text)


def test_the_four_files_refuse_nothing_themselves():
    """Every refusal of the eight entries comes from the one check: the files that hold them have no argument check of their own, and
    every entry and every size function goes through the header.  (What the check says is held by the table, the sizes and the limits
    above; that it needs no HIP is held by the build of rows_check_pure.cpp, which refuses to compile under HIP.)"""
    code = {name: _code((CSRC / name).read_text()) for name in FILES}
    for name, text in code.items():
        assert not re.search(r"\bSD_CHECK_ARG\(|\bsd_set_error\(", text), name
    assert sum(len(re.findall(r"\bsd_rows_refused\(", text)) for text in code.values()) == len(R.NAME)
    assert sum(len(re.findall(r"\bsd_rows_workspace_bytes\(", text)) for text in code.values()) == len(R.HAS_WS)
