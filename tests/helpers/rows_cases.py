"""One table of refused calls of the eight entries that take f32 rows (csrc/sd_rows_check.h), written out by
hand: every rule of every entry alone, and every pair of rules that are adjacent in an entry's order broken together, which must report
the earlier one.  A row is (entry, arguments that differ from DEFAULT, status code, the full text of sd_last_error).

Three readers: tests/test_rows_check_rules.py hands the rows to the header alone (tests/helpers/rows_check_pure.cpp) and to the built
library, tools/rows_check_parity.py to the parent's library and this one.  Every row is a refusal: the pointers are invented
(`call_library`), so a call that passed its check would launch on them."""
ARG, UNSUP, WS = -1, -2, -3          # SD_ERR_ARG, SD_ERR_UNSUPPORTED, SD_ERR_WORKSPACE (include/sd_hip.h)

NAME = {"nearest": "sd_ahc_nearest_f32", "merge": "sd_ahc_merge_f32", "grouped": "sd_ahc_nearest_grouped_f32", "core": "sd_hdb_core_f32",
        "outgoing": "sd_hdb_outgoing_f32", "stats": "sd_whiten_stats_f64", "apply": "sd_whiten_apply_f64", "centroids": "sd_label_centroids_f32"}
OPERAND = {"nearest": "sums", "merge": "sums", "grouped": "sums", "core": "rows", "outgoing": "rows", "stats": "x", "apply": "x", "centroids": "x"}
# k: max_group of the grouped entry.  ld2, ld3: ldg | ldw, ldo | ldo.  ws None: what the call needs.
# flags: p = a null pointer, r = rows 4 bytes off, m = workspace 4 bytes off
DEFAULT = dict(n=100, d=192, ld=192, k=0, ld2=192, ld3=192, ws=None, flags="")
DEFAULT_K = {"grouped": 40, "core": 2, "centroids": 4}
HAS_WS = ("nearest", "grouped", "core", "outgoing", "stats")

BIG_N = 65535 * 128 + 1              # one row past the last tile of a grid: 65 536 tiles
WIDE = dict(d=1025, ld=1028)         # past GT_MAX_D
WIDE_DG = dict(d=257, ld=260, ld2=260, ld3=260)     # past DG_MAX_D


def _rows_then_pointers(e, shape, last_shape):
    """The rules every entry shares from the null pointer on; `shape`: the text of n / d / ld at n = 0; `last_shape`: (arguments, code,
    text) of the entry's last rule before the pointers."""
    al = f"{OPERAND[e]} must be 16-byte aligned with ld % 4 == 0"
    args, code, text = last_shape
    return [
        (e, dict(n=0), ARG, shape),
        (e, dict(args, flags="p"), code, text),
        (e, dict(flags="p"), ARG, "null pointer"),
        (e, dict(flags="pr"), ARG, "null pointer"),
        (e, dict(flags="p", d=190, ld=190), ARG, "null pointer"),
        (e, dict(flags="r"), ARG, f"{al} (ld=192)"),
        (e, dict(d=190, ld=190), ARG, f"{al} (ld=190)"),
        (e, dict(d=7, ld=9), ARG, f"{al} (ld=9)"),
    ]


def _workspace(e, tail, need, limit):
    """... and from the workspace's alignment on; `tail`: what the size message adds after d; `limit`: (arguments, text) of the grid limit."""
    al = f"{OPERAND[e]} must be 16-byte aligned with ld % 4 == 0"
    out = [
        (e, dict(flags="rm"), ARG, f"{al} (ld=192)"),
        (e, dict(flags="m"), ARG, "workspace is not 16-byte aligned"),
        (e, dict(flags="m", ws=0), ARG, "workspace is not 16-byte aligned"),
        (e, dict(ws=need - 1), WS, f"workspace of {need - 1} bytes, n=100 d=192{tail} needs {need}"),
        (e, dict(ws=0), WS, f"workspace of 0 bytes, n=100 d=192{tail} needs {need}"),
    ]
    if limit:
        args, text = limit
        out += [(e, dict(args, flags="m"), ARG, "workspace is not 16-byte aligned"), (e, args, UNSUP, text), (e, dict(args, ws=0), UNSUP, text)]
    return out


def _table():
    t = []
    too_wide = "d=1025, at most 1024 columns are supported"
    too_many = (dict(n=BIG_N), f"n={BIG_N}, at most 8388480 rows are supported")
    for e in ("nearest", "outgoing"):
        t += _rows_then_pointers(e, "n=0 d=192 ld=192", (WIDE, UNSUP, too_wide))
        t += [(e, dict(n=-5), ARG, "n=-5 d=192 ld=192"), (e, dict(d=0), ARG, "n=100 d=0 ld=192"), (e, dict(d=-1), ARG, "n=100 d=-1 ld=192"),
              (e, dict(ld=188), ARG, "n=100 d=192 ld=188"), (e, dict(WIDE, n=0), ARG, "n=0 d=1025 ld=1028"), (e, WIDE, UNSUP, too_wide)]
        t += _workspace(e, "", 2048, too_many)

    e = "merge"                      # no limit on d, no workspace
    t += _rows_then_pointers(e, "n=0 d=192 ld=192", (dict(ld=188), ARG, "n=100 d=192 ld=188"))
    t += [(e, dict(d=0), ARG, "n=100 d=0 ld=192"), (e, dict(ld=188), ARG, "n=100 d=192 ld=188")]

    e = "grouped"
    t += _rows_then_pointers(e, "n=0 d=192 ld=192", (dict(k=0), ARG, "max_group=0"))
    t += [(e, dict(d=0), ARG, "n=100 d=0 ld=192"), (e, dict(ld=188), ARG, "n=100 d=192 ld=188"), (e, dict(WIDE, n=0), ARG, "n=0 d=1025 ld=1028"),
          (e, WIDE, UNSUP, too_wide), (e, dict(WIDE, k=0), UNSUP, too_wide), (e, dict(k=0), ARG, "max_group=0"), (e, dict(k=-3), ARG, "max_group=-3")]
    # W = min(T - 1, ceil((max_group - 1) / 128)) reaches 65 535 at 65 536 tiles and max_group = 65 534 * 128 + 2
    t += _workspace(e, " max_group=40", 2048, (dict(n=BIG_N, k=65534 * 128 + 2), "max_group=8388354, a group of at most 8388352 rows is supported"))

    e = "core"
    few = "k=17, at most 16 neighbours are supported"
    t += _rows_then_pointers(e, "n=0 d=192 ld=192", (dict(k=0), ARG, "k=0 must lie in 1 .. n - 1 (n=100)"))
    t += [(e, dict(d=0), ARG, "n=100 d=0 ld=192"), (e, dict(ld=188), ARG, "n=100 d=192 ld=188"), (e, dict(WIDE, n=0), ARG, "n=0 d=1025 ld=1028"),
          (e, WIDE, UNSUP, too_wide), (e, dict(WIDE, k=17), UNSUP, too_wide), (e, dict(k=17), UNSUP, few), (e, dict(k=17, n=10), UNSUP, few),
          (e, dict(k=0), ARG, "k=0 must lie in 1 .. n - 1 (n=100)"), (e, dict(k=-1), ARG, "k=-1 must lie in 1 .. n - 1 (n=100)"),
          (e, dict(k=10, n=10), ARG, "k=10 must lie in 1 .. n - 1 (n=10)"), (e, dict(k=1, n=1), ARG, "k=1 must lie in 1 .. n - 1 (n=1)")]
    t += _workspace(e, " k=2", 1024, too_many)

    e = "stats"                      # 1 block of 512 rows, T = 12: (16 * 12 + 256 * 78) * 8 bytes
    note = " (n >= 2: one row has no covariance)"
    too_wide = "d=257, at most 256 columns are supported"
    t += _rows_then_pointers(e, "n=0 d=192 ld=192 ldg=192" + note, (WIDE_DG, UNSUP, too_wide))
    t += [(e, dict(n=1), ARG, "n=1 d=192 ld=192 ldg=192" + note), (e, dict(d=0), ARG, "n=100 d=0 ld=192 ldg=192" + note),
          (e, dict(ld=188), ARG, "n=100 d=192 ld=188 ldg=192" + note), (e, dict(ld2=191), ARG, "n=100 d=192 ld=192 ldg=191" + note),
          (e, dict(WIDE_DG, n=1), ARG, "n=1 d=257 ld=260 ldg=260" + note), (e, WIDE_DG, UNSUP, too_wide)]
    t += _workspace(e, "", 161280, None)

    e = "apply"
    t += _rows_then_pointers(e, "n=0 d=192 ld=192 ldw=192 ldo=192", (WIDE_DG, UNSUP, too_wide))
    t += [(e, dict(d=0), ARG, "n=100 d=0 ld=192 ldw=192 ldo=192"), (e, dict(ld=188), ARG, "n=100 d=192 ld=188 ldw=192 ldo=192"),
          (e, dict(ld2=191), ARG, "n=100 d=192 ld=192 ldw=191 ldo=192"), (e, dict(ld3=100), ARG, "n=100 d=192 ld=192 ldw=192 ldo=100"),
          (e, dict(WIDE_DG, n=0), ARG, "n=0 d=257 ld=260 ldw=260 ldo=260"), (e, WIDE_DG, UNSUP, too_wide)]

    e = "centroids"
    many = "k=1025, at most 1024 labels are supported"
    t += _rows_then_pointers(e, "n=0 d=192 k=4 ld=192 ldo=192", (dict(k=1025), UNSUP, many))
    t += [(e, dict(d=0), ARG, "n=100 d=0 k=4 ld=192 ldo=192"), (e, dict(k=0), ARG, "n=100 d=192 k=0 ld=192 ldo=192"),
          (e, dict(ld=188), ARG, "n=100 d=192 k=4 ld=188 ldo=192"), (e, dict(ld2=191), ARG, "n=100 d=192 k=4 ld=192 ldo=191"),
          (e, dict(WIDE_DG, k=0), ARG, "n=100 d=257 k=0 ld=260 ldo=260"), (e, WIDE_DG, UNSUP, too_wide), (e, dict(WIDE_DG, k=1025), UNSUP, too_wide),
          (e, dict(k=1025), UNSUP, many)]
    return [(e, a, code, f"{NAME[e]}: {text}") for e, a, code, text in t]


REFUSALS = _table()


def arguments(entry, args):
    """DEFAULT with the entry's k and `args`."""
    return {**DEFAULT, "k": DEFAULT_K.get(entry, 0), **args}


def pure_spec(entry, args):
    """The row as an argument of tests/helpers/rows_check_pure.cpp."""
    a = arguments(entry, args)
    return f"{entry}:{a['n']}:{a['d']}:{a['ld']}:{a['k']}:{a['ld2']}:{a['ld3']}:{-1 if a['ws'] is None else a['ws']}:{a['flags'] or '-'}"


def call_library(lib, entry, args):
    """The row as a call of the loaded library, on invented pointers (never followed by a call that is refused) -> the status code."""
    a = arguments(entry, args)
    n, d, ld, k = a["n"], a["d"], a["ld"], a["k"]
    rows = 0x1000 + (4 if "r" in a["flags"] else 0)
    p = None if "p" in a["flags"] else 0x2000        # the first pointer after the rows
    ws = 0x9000 + (4 if "m" in a["flags"] else 0)
    if a["ws"] is not None:
        ws_bytes = a["ws"]
    elif entry in HAS_WS:
        size = {"nearest": lib.sd_ahc_nearest_workspace_bytes, "outgoing": lib.sd_hdb_outgoing_workspace_bytes, "stats": lib.sd_whiten_stats_workspace_bytes,
                "grouped": lib.sd_ahc_nearest_grouped_workspace_bytes, "core": lib.sd_hdb_core_workspace_bytes}[entry]
        ws_bytes = int(size(n, d, k) if entry in ("grouped", "core") else size(n, d))
    if entry == "nearest":
        return lib.sd_ahc_nearest_f32(rows, ld, n, d, p, 0x3000, 0x4000, ws, ws_bytes, None)
    if entry == "merge":
        return lib.sd_ahc_merge_f32(rows, ld, n, d, p, 0x3000, 0x4000, 0x5000, 0.7, 0x6000, 0x7000, None)
    if entry == "grouped":
        return lib.sd_ahc_nearest_grouped_f32(rows, ld, n, d, p, 0x3000, k, 0x4000, 0x5000, 0x6000, ws, ws_bytes, None)
    if entry == "core":
        return lib.sd_hdb_core_f32(rows, ld, n, d, k, p, ws, ws_bytes, None)
    if entry == "outgoing":
        return lib.sd_hdb_outgoing_f32(rows, ld, n, d, p, 0x3000, 0x4000, 0x5000, ws, ws_bytes, None)
    if entry == "stats":
        return lib.sd_whiten_stats_f64(rows, ld, n, d, p, 0x3000, a["ld2"], ws, ws_bytes, None)
    if entry == "apply":
        return lib.sd_whiten_apply_f64(rows, ld, n, d, p, 0x3000, a["ld2"], 1e-9, 0x4000, a["ld3"], None)
    assert entry == "centroids", entry
    return lib.sd_label_centroids_f32(rows, ld, n, d, p, k, 1e-9, 0x3000, a["ld2"], 0x4000, None)
