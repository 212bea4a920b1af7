"""Arguments for `sd_conv_choice_read` (include/sd_hip_trace.h) without a device: `sd_conv_args` over made-up aligned addresses, the
arguments tests/test_gpu_exact.py::run_conv builds for a case of exact_cases.py, the tile count a label stands for, and -- for the GPU
-- a recorder that asks the choice for the very arguments a conv entry is called with.

Imported as a helper (tests/helpers on sys.path), by tests/test_conv_choice_rules.py, tests/test_gpu_exact.py and tools/conv_choice_census.py."""
import collections
import contextlib
import ctypes as C
import re

import exact_cases as E
from kernel_selection import CONV_KERNELS

ADDR = 0x7F0000001000        # 16-byte aligned, never dereferenced: a choice looks at null / not null and at the alignment only
F32, F16, SPLIT = 0, 1, 2    # SD_DT_*
ACT = {None: 0, "relu": 1, "tanh": 2, "sigmoid": 3}


def conv_args(M, T, cin, cout, *, cin_pad=None, taps=1, dil=1, lda=None, a_col0=0, ldo=None, o_col0=0, x=F32, w=F32, y=F32, act="relu", act2=None,
              bias_per_seg=False, tee=None, tee_add=False, colstat=False):
    """An sd_conv_args of that shape.  tee: (tee_lo, tee_hi) or None; every pointer that is set is ADDR plus a multiple of 4096."""
    from speech_diarization_amd import _native as N
    a = N.sd_conv_args()
    a.x, a.w, a.y = ADDR, ADDR + 4096, ADDR + 8192
    a.bias, a.scale, a.shift = ADDR + 12288, ADDR + 16384, ADDR + 20480
    a.x_dtype, a.w_dtype, a.y_dtype = x, w, y
    a.M, a.T, a.cin, a.cout, a.taps, a.dil = M, T, cin, cout, taps, dil
    a.cin_pad = cin_pad if cin_pad is not None else -(-cin // 32) * 32
    a.lda, a.a_col0 = (lda if lda is not None else a_col0 + cin), a_col0
    a.ldo, a.o_col0 = (ldo if ldo is not None else o_col0 + cout), o_col0
    a.act, a.act2, a.bias_per_seg = ACT[act], ACT[act2], int(bias_per_seg)
    if tee:
        a.tee, a.tee_lo, a.tee_hi, a.ldt = ADDR + 24576, tee[0], tee[1], tee[1] - tee[0] + 8
        if tee_add:
            a.tee_add, a.ld_ta, a.ta_col0 = ADDR + 28672, tee[1] - tee[0] + 16, 8
    if colstat:
        a.colstat = ADDR + 32768
    return a


def case_args(name, op, x16=False, y16=False, split_out=False, colstat=False):
    """What run_conv (tests/test_gpu_exact.py) hands the entry for case `name` of exact_cases.py through `op` in {"f32", "packed",
    "seg", "f16", "narrow", "wide"}: x framed by 8 columns, y at column 8 of a row 24 wider than cout; the wide split form over the packed
    x (cin_pad columns from 0) and, with split_out, y as SD_DT_SPLIT16 at column 0 of a row of cout + 32 values."""
    shape, _, what = name.partition("-")
    if shape[0] == "C":
        bt, cout = name[1:].split("-")
        B, T = (int(v) for v in bt.split("x"))
        s = dict(B=B, T=T, cin=64, cout=int(cout), k=1, dil=1)
        epi = (False, "relu", None, False)
        colstat = True
    else:
        s = E.SHAPES[shape]
        epi = E.DENSE[name] if name in E.DENSE else (False, None, E.GATHER_TEE.get(name), False)
    per_seg, act, tee, add = epi
    M = sum(s["spans"]) if "spans" in s else s["B"] * s["T"]
    T = M if "spans" in s else s["T"]
    cin, cout, k, dil = s["cin"], s["cout"], s["k"], s["dil"]
    kw = dict(taps=k, dil=dil, act=act, bias_per_seg=per_seg, tee=tee, tee_add=add, colstat=colstat, lda=cin + 16, a_col0=8, ldo=cout + 24, o_col0=8)
    if op == "seg":
        return conv_args(M, 1, cin, cout, act=act, lda=cin + 16, ldo=cout + 24)
    if op in ("f32", "packed"):
        return conv_args(M, T, cin, cout, **kw)
    if op == "f16":
        return conv_args(M, T, cin, cout, cin_pad=-(-cin // 64) * 64, x=F16 if x16 else F32, w=F16, y=F16 if y16 else F32, **kw)
    if split_out:
        kw.update(ldo=cout + 32, o_col0=0)
    if op == "narrow":
        return conv_args(M, T, cin, cout, w=SPLIT, y=SPLIT if split_out else F32, **kw)
    cp = -(-cin // 32) * 32
    kw.update(lda=cp, a_col0=0)
    return conv_args(M, T, cin, cout, cin_pad=cp, x=SPLIT, w=SPLIT, y=SPLIT if split_out else F32, **kw)


def tile_count(label, a):
    """The grid a label's tile size gives for the shape of `a`; None for the symmetric band list.  The seg_gemm pair: the partial
    kernel has one workgroup per 32x32 tile and K split, the reduction four per tile."""
    cd = lambda p, q: -(-p // q)  # noqa: E731
    if label.endswith("/lockstep"):
        return 256
    if label.endswith("/symmetric"):
        return None
    m = re.match(r"conv_gemm_f32_(?:s64|vh)_kernel<(\d+)>", label)
    if m:
        rows, cols = (int(m.group(1)), 64) if "s64" in label else (16 * int(m.group(1)), 128)
    elif label.startswith("seg_gemm_"):
        groups = 8 if a.cin_pad >= 2048 else 4
        return cd(a.M, 32) * cd(a.cout, 32) * (cd(a.cin_pad, 32 * groups) if "partial" in label else 4)
    else:
        rows, cols = {"skinny_gemm_f32_kernel": (32, 32), "conv_gemm_f32_t256_kernel": (256, 256), "conv_gemm_f16_t256_kernel": (256, 256),
                      "conv_gemm_f32_n64_kernel": (128, 64)}.get(E.kernel_of(label), (128, 128))
    return cd(a.M, rows) * cd(a.cout, cols)


def check_line(line, a, what=""):
    """What every choice must satisfy (the issue's "grid and LDS")."""
    label, grid, block, lds, stat_rows = line
    want = tile_count(label, a)
    assert grid >= 1 and (want is None or grid == want), (what, line, want)
    assert block in (256, 512) and 0 <= lds <= 160 * 1024, (what, line)
    assert stat_rows in (128, 80, 96, 112) and (stat_rows == 128 or label == f"conv_gemm_f32_vh_kernel<{stat_rows // 16}>"), (what, line)
    if "vh_kernel" in label:
        assert stat_rows == 16 * int(label[-2]), (what, line)


# ---- what tests/test_gpu_exact.py::test_the_choice_is_what_ran launches (and tools/conv_choice_census.py with it).
# The smallest shapes on both sides of each rule of the choice layer (csrc/sd_conv_choice.h).  r*: the ring / skinny edge (M = 262 and 64
# take the 64x64 ring kernel, M = 63 < 64 rows the 32x32 one); p*: 262 and 704 rows at cout 1016 / 1024 for the rows80 / rows96 / rows112,
# tiles64 and wide256 pins (cout 1016 < 1024 never takes a 256x256 kernel, and has a ragged last column tile); w40 / w41: 40 / 41 segments
# of T = 201 at cout 1024 are 128 / 132 tiles of 256x256, the two sides of SD_TUNE_F16_NARROW_TILES; g*: sd_seg_gemm_f32 at cin_pad 480 /
# 512 (K too short / long enough to split) and M 256 / 257 (the last M that splits / the first that does not).
CHOICE_SHAPES = {
    "r262": dict(B=2, T=131, cin=32, cout=72, k=3, dil=1), "r64": dict(B=1, T=64, cin=32, cout=72, k=3, dil=1),
    "r63": dict(B=7, T=9, cin=32, cout=72, k=3, dil=1),
    "p262-1016": dict(B=2, T=131, cin=32, cout=1016, k=1, dil=1), "p262-1024": dict(B=2, T=131, cin=32, cout=1024, k=1, dil=1),
    "p704-1016": dict(B=4, T=176, cin=32, cout=1016, k=1, dil=1), "p704-1024": dict(B=4, T=176, cin=32, cout=1024, k=1, dil=1),
    "w40": dict(B=40, T=201, cin=64, cout=1024, k=1, dil=1), "w41": dict(B=41, T=201, cin=64, cout=1024, k=1, dil=1),
    "g256-480": dict(B=256, T=1, cin=480, cout=40, k=1, dil=1), "g257-480": dict(B=257, T=1, cin=480, cout=40, k=1, dil=1),
    "g256-512": dict(B=256, T=1, cin=512, cout=40, k=1, dil=1), "g257-512": dict(B=257, T=1, cin=512, cout=40, k=1, dil=1),
    "spans": dict(spans=(5, 7, 131, 9, 110), cin=32, cout=72, k=3, dil=1),
}


def _f32_runs(shape):
    return [("f32", shape, sel, {}) for sel in CONV_KERNELS]


CHOICE_RUNS = {
    **{f"f32-{s}": _f32_runs(s) for s in ("r262", "r64", "r63", "p262-1016", "p262-1024", "p704-1016", "p704-1024")},
    **{f"f32-{s}": [("f32", s, sel, {}) for sel in ("auto", "wide256")] for s in ("w40", "w41")},
    **{f"seg-{s}": [("seg", s, "auto", {})] for s in CHOICE_SHAPES if s[0] == "g"},
    "packed-spans": [("packed", "spans", "auto", {})],
    **{f"f16-{s}": [("f16", s, "auto", dict(f16_tiles=t, lockstep=lk, x16=x, y16=y)) for t in (-1, 0) for lk in (-1, 0) for x, y in ((1, 1), (1, 0), (0, 1))]
       for s in ("p262-1016", "p262-1024", "w40", "w41")},
    "narrow-r262": [("narrow", "r262", "auto", {})],
    **{f"wide-{s}": [("wide", s, "auto", dict(lockstep=lk)) for lk in (-1, 0)] for s in ("p262-1016", "p262-1024", "w41")},
}


ENTRIES = {"sd_conv1d_cl_f32": "f32", "sd_conv1d_cl_f16": "f16", "sd_conv1d_cl_split16": "split16", "sd_conv1d_cl_packed_f32": "packed",
           "sd_seg_gemm_f32": "seg_gemm"}


@contextlib.contextmanager
def predicted_launches(n_cu):
    """Inside the scope every call of a public conv entry through the loaded library first asks sd_conv_choice_read what the entry would
    launch for the SAME sd_conv_args (and scratch size) on a device of n_cu CUs; yields the Counter of the predicted labels, and the list
    of (entry, lines)."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    count, calls = collections.Counter(), []
    real = {name: getattr(lib, name) for name in ENTRIES}

    def wrap(name):
        def call(args, *rest):
            scratch = rest[1] if name == "sd_seg_gemm_f32" and rest[0] else 0
            lines = N.conv_choice_read(args._obj, ENTRIES[name], n_cu, scratch)
            for ln in lines:
                check_line(ln, args._obj, name)
            count.update(ln[0] for ln in lines)
            calls.append((name, lines))
            return real[name](args, *rest)
        return call
    try:
        for name in ENTRIES:
            setattr(lib, name, wrap(name))
        yield count, calls
    finally:
        for name, fn in real.items():
            setattr(lib, name, fn)
