"""Exact known-answer tests of every matrix-core and reduction kernel: inputs on which no product and no sum rounds (small integers,
powers of two, one-hot weights; tests/helpers/exact_cases.py checks every case's bit budget on the host), so that the integer reference
gives the BITS a kernel must produce whatever its tile shape, K order, split-K order or MFMA form.  Every assertion is `torch.equal`;
the only tolerance in this file is the rtol on sqrt(eps) = sqrt(1e-12f) of a constant column (1e-6 to f32 rounding, the bar of
test_std_clamp_on_constant_input).  Output buffers are pre-filled with NaN and are wider than the slice a kernel may write; the columns
outside the slice must keep their NaN.  Input rows are wider than the slice a kernel may read, NaN outside it.

Conv shapes (B, T, cin, cout, k, dil) and what they cross:
  S1  3, 57, 36, 72, 3, 2      M = 171 crosses 32, 64, 80, 96, 112 and 128 rows; cout = 64 + 8; a K tail of 4
  S2  2, 131, 80, 1032, 5, 1   M = 256 + 6; cout = 1024 + 8 qualifies for the 256x256 kernels; the stem's cin_pad
  S3  5, 9, 128, 100, 3, 4     pad 4 just under T; several segment boundaries per tile; cout % 8 != 0: the scalar epilogue
  S4  70, 1, 544, 40, 1, 1     T = 1; through sd_seg_gemm_f32 a grid split-K whose last split is ragged
  P   spans 5, 7, 5, 9, 131 with S1's channels (sd_conv1d_cl_packed_f32)
  H1 / H2 / H2w / H2L / H3: S1 .. S3 for sd_conv1d_cl_f16 (which takes activations in groups of 8 channels and refuses S1's 36: 40
  there; H2w: cout 1100; H2L: cout 1024 = four column tiles of 256, which the lockstep walk of the 256x256 kernel needs: 1032 gives
  five), N128 / W1032 / W256 / W1024: the narrow and wide forms of sd_conv1d_cl_split16, C*: the column statistics.
  S5  8, 128, 32, 512, 3, 2    32 tiles of 128x128 but 128 of 64x64: the 64-row form of the 64x64 ring kernel, which S1 .. S3 never reach

Every test body takes an exponent `e` (default 0, and 0 in every test of this file): tests/test_gpu_scale.py runs the same bodies on the
twins at 2^e (tests/helpers/exact_cases.py), so a twin sees the shapes, selections, buffers and launch labels of its unscaled case.

Every run is held to the launch label it must take (tests/helpers/launch_log.py; the labels per case, selection, storage type and
tuning are stated in tests/helpers/exact_cases.py): the conv operators to exactly that label and no other kernel of the operator, the
reductions and products to at least the labels named.

Left out, each because the operation is inexact by construction (a reason the issue allows):
  * `asnorm_combine`: divides by std + 1e-6, no power of two.
  * column statistics under the 80 / 96 / 112-row kernels: sd_conv1d_cl_f32 takes those tiles only WITHOUT a colstat (the public entry
    writes units of 128 rows); `sd_colstat_finish_rows` is reached by the forward alone, whose tanh / sigmoid are inexact.  The "rowsNN"
    selections are run all the same: they must fall back to the 128-row units and give the same bits.
  * `topk_mean_std` with k = n for n in {50, 257, 1000}: the mean divides by n, no power of two, so only rows whose quotient is an
    integer are asserted, and the std only where sum of squares / k is the square of a dyadic number.
  * uniform non-zero logits in the FUSED pooling kernels: they form the exponent as acc * log2(e) + (-max * log2(e)) with the second
    product rounded on its own, so equal logits give exp2 of a rounding residual, not exp2(0); the fused uniform case uses logits 0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ahc_ref  # noqa: E402
import exact_cases as E  # noqa: E402
from conv_choice import CHOICE_RUNS, CHOICE_SHAPES, predicted_launches  # noqa: E402
from kernel_selection import CONV_KERNELS, f16_tiles, restore_conv_kernel, select_conv_kernel  # noqa: E402,F401
from launch_log import F16_CONV, F32_CONV, SPLIT_CONV, expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16
NAN = float("nan")


# ------------------------------------------------------------------ plumbing

def _dev(a, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype).to(dev)


def _framed(a, dtype, dev, left=8, right=8):
    """a [M, C] inside a NaN buffer [M, left + C + right] -> (buffer, the view of the C columns)."""
    M, Cc = a.shape
    buf = torch.full((M, left + Cc + right), NAN, dtype=dtype, device=dev)
    buf[:, left:left + Cc] = _dev(a, dtype, dev)
    return buf, buf[:, left:left + Cc]


def _same(got, want, what):
    """Bit equality (torch.equal); a mismatch reports where, and what was read there."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        idx = bad.nonzero()
        first = tuple(int(v) for v in idx[0])
        pytest.fail(f"{what}: {idx.shape[0]} of {got.numel()} values differ; first at {first}: got {got[first].item()!r}, "
                    f"want {want[first].item()!r}; rows {sorted(set(idx[:, 0].tolist()))[:12]}")


def _untouched(buf, lo, hi, what):
    assert bool(torch.isnan(buf[:, :lo]).all()) and bool(torch.isnan(buf[:, hi:]).all()), f"{what}: wrote outside columns [{lo}, {hi})"


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from speech_diarization_amd import _native as N
    return N, N.load()


def run_conv(dev, c, op, xdt=F32, ydt=F32, split_out=False, colstat=None):
    """One launch of case `c` through `op` in {"f32", "packed", "seg", "f16", "narrow", "wide"} -> dict(y, tee) of the slices written,
    after checking that nothing outside them was."""
    from speech_diarization_amd import ops
    M, cin, cout = c.M, c.cin, c.cout
    xbuf, _ = _framed(c.x, xdt, dev)
    o0 = 8
    ybuf = torch.full((M, o0 + cout + 16), NAN, dtype=ydt, device=dev)
    vec = lambda v: None if v is None else _dev(v, F32, dev)  # noqa: E731
    kw = dict(cin=cin, bias=vec(c.bias), act=c.act, scale=vec(c.scale), shift=vec(c.shift))
    tee = None
    if op != "seg":
        kw.update(dil=c.dil, bias_per_seg=c.bias_per_seg, a_col0=8)
        if c.tee_hi:
            tee = torch.full((M, c.tee_hi - c.tee_lo + 8), NAN, dtype=ydt, device=dev)
            kw.update(tee=tee, tee_lo=c.tee_lo, tee_hi=c.tee_hi)
            if c.tee_add is not None:
                tabuf, _ = _framed(c.tee_add, ydt, dev)
                kw.update(tee_add=tabuf, ta_col0=8)
    ysp = None
    if split_out:
        ysp = torch.full((M, 2 * (cout + 32)), NAN, dtype=F16, device=dev)
    if op == "f32":
        ops.conv1d_cl(xbuf, ops.pack_weight(c.w, dev), c.T, out=ybuf, o_col0=o0, colstat=colstat, **kw)
    elif op == "packed":
        ops.conv1d_cl_packed(xbuf, ops.pack_weight(c.w, dev), c.frame_start, out=ybuf, o_col0=o0, **kw)
    elif op == "seg":
        ops.seg_gemm(xbuf[:, 8:8 + cin], ops.pack_weight(c.w, dev), out=ybuf[:, o0:o0 + cout], **kw)
    elif op == "f16":
        ops.conv1d_cl(xbuf, ops.pack_weight(c.w, dev, F16), c.T, out=ybuf, o_col0=o0, colstat=colstat, **kw)
    else:
        ws, s = ops.pack_weight_split16(c.w, dev)
        ops.conv1d_cl_split16(xbuf, ws, s, c.T, narrow=op == "narrow", out=ybuf, o_col0=0 if split_out else o0, out_split=ysp,
                              colstat=colstat, **kw)
    torch.cuda.synchronize()
    got = {}
    if split_out:
        assert bool(torch.isnan(ybuf).all()) and bool(torch.isnan(ysp[:, 2 * cout:]).all()), f"{c.name}: wrote outside the split slice"
        got["ysplit"] = ysp[:, :2 * cout]
    else:
        _untouched(ybuf, o0, o0 + cout, c.name + " y")
        got["y"] = ybuf[:, o0:o0 + cout]
    if tee is not None:
        _untouched(tee, 0, c.tee_hi - c.tee_lo, c.name + " tee")
        got["tee"] = tee[:, :c.tee_hi - c.tee_lo]
    return got


def check_conv(dev, c, got, ydt, what):
    from speech_diarization_amd import ops
    what = f"{c.name} {what}"
    if "ysplit" in got:        # bit for bit what sd_split16_pack_f32 makes of the integer answer, and what the header's rule makes of it in numpy
        _same(got["ysplit"], ops.split16_pack(_dev(c.y, F32, dev), 0, c.cout), what + " y (split)")
        _same(got["ysplit"], torch.from_numpy(E.split16_rows(c.y)), what + " y (split, numpy pack)")
    else:
        _same(got["y"], _dev(c.y, ydt, dev), what + " y")
    if c.tee_hi:
        _same(got["tee"], _dev(c.tee, ydt, dev), what + " tee")


def _launches(kind):
    N, _ = _lib()
    return N.profile_read(kind)[1]


def test_launch_log_counts_and_reports_a_short_buffer(dev):
    """Two launches under two labels: the counts, the text of sd_launch_log_read, and a buffer shorter than the text -- the result
    is the bytes the whole text needs (above cap), and the truncated copy is still terminated."""
    from launch_log import launches
    from speech_diarization_amd import ops
    N, lib = _lib()
    x = torch.ones(5, 8, device=dev)
    with launches() as log:
        ops.l2norm_rows(x)
        ops.l2norm_rows(x)
        ops.adjacent_cosine(x, eps=0.0)
        text = b"adjacent_cosine_kernel\t1\nl2norm_rows_kernel\t2\n"
        full = C.create_string_buffer(b"x" * 64, 64)
        assert int(lib.sd_launch_log_read(full, 64)) == len(text) + 1 and full.value == text
        small = C.create_string_buffer(b"xxxxxx", 6)
        assert int(lib.sd_launch_log_read(small, 4)) == len(text) + 1 > 4
        assert small.raw[:4] == b"adj\0" and small.raw[4:] == b"xx"          # cap - 1 bytes and the NUL; nothing past cap
    assert log == {"adjacent_cosine_kernel": 1, "l2norm_rows_kernel": 2}
    assert N.launch_log_enable(False) is False and N.launch_log_read() == log        # off again; the counts stay readable


# ------------------------------------------------------------------ 1. convs

F32_CASES = [n for n in E.CONV_CASE_NAMES if n[0] == "S"]


@pytest.mark.parametrize("name", F32_CASES)
def test_conv1d_cl_f32_every_selection_gives_the_integers(dev, name, e=0):
    """All eight selections of the exact-f32 operator must give the reference's bits, hence each other's.  S2 under "wide256" must have
    launched the 256x256 kernel; S4 also goes through sd_seg_gemm_f32, whose grid split-K (cin_pad = 544: five splits of 128, the last
    ragged) must have run.  (`e`, here and below: the twin at 2^e that tests/test_gpu_scale.py runs through the same body.)"""
    N, _ = _lib()
    c = E.conv_case(name, e)
    try:
        for sel in CONV_KERNELS:
            select_conv_kernel(sel)
            N.profile_enable(True)
            with expect_launches(exactly=[E.F32_LABELS[name.split("-")[0]][sel]], family=F32_CONV):
                got = run_conv(dev, c, "f32")
            wide = _launches(N.SD_PROF_CONV_WIDE)
            N.profile_enable(False)
            check_conv(dev, c, got, F32, sel)
            if name.startswith("S2") and sel == "wide256":
                assert wide == 1, f"{name}: the 256x256 kernel was not launched ({wide})"
    finally:
        N.profile_enable(False)
        restore_conv_kernel()
    if name.startswith("S4"):
        N.profile_enable(True)
        with expect_launches(exactly=E.SEG_GEMM_LABELS, family=F32_CONV):
            got = run_conv(dev, c, "seg")
        n_split = _launches(N.SD_PROF_SEG_SPLITK)
        N.profile_enable(False)
        check_conv(dev, c, got, F32, "seg_gemm")
        assert n_split == 1, f"{name}: sd_seg_gemm_f32 did not split K over the grid ({n_split})"


@pytest.mark.parametrize("name", ["P-rows", "P-chan", "P-dense"])
def test_conv1d_cl_packed_f32_gives_the_integers(dev, name, e=0):
    """Spans 5, 7, 5, 9, 131: "P-rows" returns the source row of every tap, so a tap that crossed a span edge names the row it read;
    "P-dense" carries a bias per span."""
    c = E.conv_case(name, e)
    with expect_launches(exactly=[E.PACKED_LABEL], family=F32_CONV):
        got = run_conv(dev, c, "packed")
    check_conv(dev, c, got, F32, "packed")


F16_CASES = [n for n in E.CONV_CASE_NAMES if n[0] == "H"]


@pytest.mark.parametrize("name", F16_CASES)
def test_conv1d_cl_f16_gives_the_integers(dev, f16_tiles, name, e=0):
    """f16 and f32 x, f16 and f32 y, under both tile choices; the cout >= 1024 cases also with SD_TUNE_T256_LOCKSTEP_TILES = 0, which
    makes H2L (register epilogue, four column tiles) take the lockstep walk of the 256x256 kernel from its first tile: hardware dispatch
    and lockstep must both give the integers.  H2-dense takes the register epilogue, H2-dense-tee / H2w-dense-tee
    (cout 1032 / 1100, per-segment bias, a tee) the staged one."""
    N, lib = _lib()
    c = E.conv_case(name, e)
    for xdt in (F16, F32):
        for ydt in (F16, F32):
            with expect_launches(exactly=[E.f16_label(name, f16_tiles, xdt == F16, ydt == F16)], family=F16_CONV):
                got = run_conv(dev, c, "f16", xdt, ydt)
            check_conv(dev, c, got, ydt, f"{f16_tiles} x {xdt} y {ydt}")
    if c.cout >= 1024:
        N.check(lib.sd_set_tuning(N.SD_TUNE_T256_LOCKSTEP_TILES, 0), "sd_set_tuning")
        try:
            for ydt in (F16, F32):
                with expect_launches(exactly=[E.f16_label(name, f16_tiles, True, ydt == F16, lockstep=True)], family=F16_CONV):
                    got = run_conv(dev, c, "f16", F16, ydt)
                check_conv(dev, c, got, ydt, f"{f16_tiles} lockstep y {ydt}")
        finally:
            N.check(lib.sd_set_tuning(N.SD_TUNE_T256_LOCKSTEP_TILES, -1), "sd_set_tuning")


@pytest.mark.parametrize("name", [n for n in E.CONV_CASE_NAMES if n[0] in "NW"])
def test_conv1d_cl_split16_gives_the_integers(dev, name, e=0, side="x"):
    """Wide form (x packed by sd_split16_pack_f32, cout 1032 and 256) and narrow form (f32 x, cout 128, full tee + tee_add, per-segment
    bias): y as f32 and, where cout % 32 == 0, as SD_DT_SPLIT16 -- the bits sd_split16_pack_f32 makes of the integer answer.  The
    2049 s operands sit on the activations ("split_x": lo.hi carries weight) and on the weights ("split_w": hi.lo does, through the
    2^s of the weight pack and w_scale_inv)."""
    N, lib = _lib()
    c = E.conv_case(name, e, side=side)
    op = "narrow" if name[0] == "N" else "wide"
    with expect_launches(exactly=E.split_labels(name), family=SPLIT_CONV):
        got = run_conv(dev, c, op)
    check_conv(dev, c, got, F32, op)
    if c.cout % 32 == 0:
        with expect_launches(exactly=E.split_labels(name, split_out=True), family=SPLIT_CONV):
            got = run_conv(dev, c, op, split_out=True)
        check_conv(dev, c, got, F32, op + " split out")
    if c.cout == 1024:      # W1024: four column tiles; SD_TUNE_T256_LOCKSTEP_TILES = 0 makes the register epilogue walk in lockstep
        N.check(lib.sd_set_tuning(N.SD_TUNE_T256_LOCKSTEP_TILES, 0), "sd_set_tuning")
        try:
            with expect_launches(exactly=E.split_labels(name, lockstep=True), family=SPLIT_CONV):
                got = run_conv(dev, c, op)
        finally:
            N.check(lib.sd_set_tuning(N.SD_TUNE_T256_LOCKSTEP_TILES, -1), "sd_set_tuning")
        check_conv(dev, c, got, F32, op + " lockstep")


_CHOICE_CASES = {}


def _choice_case(shape, kind="dense"):
    """The dense integer case of a CHOICE_SHAPES entry (per-channel bias, relu, scale, shift; x as 2049 s for the split operator),
    built once per process."""
    if (shape, kind) not in _CHOICE_CASES:
        _CHOICE_CASES[shape, kind] = E.dense_case(f"choice-{shape}-{kind}", CHOICE_SHAPES[shape], f16=kind == "dense", kind=kind, kernels=())
    return _CHOICE_CASES[shape, kind]


@pytest.mark.parametrize("runs", list(CHOICE_RUNS.values()), ids=list(CHOICE_RUNS))
def test_the_choice_is_what_ran(dev, runs):
    """Every conv entry, at the shapes on both sides of each rule and under every selection that bears on them: what the launch log
    counted is what sd_conv_choice_read said for the same sd_conv_args and this device's CU count (tests/helpers/conv_choice.py asks
    inside the entry call), label by label -- and the results are the integers, as everywhere in this file."""
    from launch_log import CONV, kernel_of, launches
    N, lib = _lib()
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    try:
        for op, shape, sel, tune in runs:
            select_conv_kernel(sel)
            N.check(lib.sd_set_tuning(N.SD_TUNE_F16_NARROW_TILES, tune.get("f16_tiles", -1)), "sd_set_tuning")
            N.check(lib.sd_set_tuning(N.SD_TUNE_T256_LOCKSTEP_TILES, tune.get("lockstep", -1)), "sd_set_tuning")
            c = _choice_case(shape, "split_x" if op in ("narrow", "wide") else "dense")
            xdt, ydt = (F16 if tune.get("x16") else F32), (F16 if tune.get("y16") else F32)
            with predicted_launches(n_cu) as (want, calls):
                with launches() as log:
                    got = run_conv(dev, c, op, xdt, ydt)
            ran = {lb: n for lb, n in log.items() if kernel_of(lb) in CONV and lb != "split16_pack_kernel"}      # (the pack pass: an entry of its own)
            assert calls and ran == dict(want), (op, shape, sel, tune, ran, dict(want))
            check_conv(dev, c, got, ydt, f"{op} {shape} {sel} {tune}")
    finally:
        restore_conv_kernel()
        N.check(lib.sd_set_tuning(N.SD_TUNE_F16_NARROW_TILES, -1), "sd_set_tuning")
        N.check(lib.sd_set_tuning(N.SD_TUNE_T256_LOCKSTEP_TILES, -1), "sd_set_tuning")


def _check_colstat(dev, c, got_y, cs, n_cs, ydt, what):
    from speech_diarization_amd import ops
    assert bool(torch.isnan(cs[n_cs:]).all()), f"{what}: wrote past the colstat buffer"
    units = E.colstat_units(c)
    want = _dev(np.nan_to_num(units), F32, dev)
    live = torch.from_numpy(~np.isnan(units)).to(dev)
    got = cs[:n_cs].view(-1, 6, c.cout)
    _same(torch.where(live, got, torch.zeros_like(got)), want, what + " raw [sum | sumsq] units")
    mean, std = E.colstat_stats(c)
    y = got_y.contiguous()
    eps = E.twin_eps(c.e)                                   # 1e-12 4^e: a constant column's std is sqrt(eps) 2^e
    with expect_launches(exactly=["colstat_finish_kernel<f16>" if ydt == F16 else "colstat_finish_kernel<f32>"]):
        st = ops.colstat_finish(cs, y, c.B, c.T, pivot=_dev(c.shift, F32, dev), want_std=True, eps=eps)
        only_mean = ops.colstat_finish(cs, y, c.B, c.T, pivot=_dev(c.shift, F32, dev), eps=eps)
    torch.cuda.synchronize()
    _same(st[:, :c.cout], _dev(mean, F32, dev), what + " mean")
    _same(only_mean, _dev(mean, F32, dev), what + " mean (no std)")
    root = float(np.ldexp(E.SQRT_EPS, c.e))
    var0 = torch.from_numpy(std == root).to(dev)
    square = torch.from_numpy(~np.isnan(std) & (std != root)).to(dev)
    got_sd = st[:, c.cout:]
    assert int(var0.sum()) > 0 and int(square.sum()) > 0
    _same(got_sd[square], _dev(std, F32, dev)[square], what + " std (perfect squares)")
    torch.testing.assert_close(got_sd[var0], torch.full_like(got_sd[var0], float(np.ldexp(1e-6, c.e))), rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("name", ["C3x128-256", "C5x64-256"])
def test_colstat_f32_gives_the_integer_sums(dev, name, e=0):
    """Under every selection ("tiles64" takes the 128x64 kernel at T >= 128; the 80 / 96 / 112-row selections must fall back to units of
    128 rows, see the module docstring)."""
    from speech_diarization_amd import ops
    c = E.conv_case(name, e, "f32")
    n_cs = ops.colstat_floats(c.M, c.cout)
    try:
        for sel in CONV_KERNELS:
            select_conv_kernel(sel)
            cs = torch.full((n_cs + 4096,), NAN, device=dev)
            with expect_launches(exactly=[E.F32_LABELS[name][sel]], family=F32_CONV):
                got = run_conv(dev, c, "f32", colstat=cs)
            check_conv(dev, c, got, F32, sel)
            _check_colstat(dev, c, got["y"], cs, n_cs, F32, f"{name} {sel}")
    finally:
        restore_conv_kernel()


@pytest.mark.parametrize("name", ["C3x128-256", "C5x64-256", "C11x64-1024", "C3x128-1024"])
def test_colstat_f16_gives_the_integer_sums(dev, f16_tiles, name, e=0):
    """cout 1024: (11, 64) is taken by the 128x128 kernel (T < 128), (3, 128) by the 256x256 kernel under "wide256"."""
    from speech_diarization_amd import ops
    c = E.conv_case(name, e, "f16")
    n_cs = ops.colstat_floats(c.M, c.cout)
    for ydt in (F16, F32):
        cs = torch.full((n_cs + 4096,), NAN, device=dev)
        with expect_launches(exactly=[E.f16_label(name, f16_tiles, True, ydt == F16)], family=F16_CONV):
            got = run_conv(dev, c, "f16", F16, ydt, colstat=cs)
        check_conv(dev, c, got, ydt, f16_tiles)
        _check_colstat(dev, c, got["y"], cs, n_cs, ydt, f"{name} f16 {f16_tiles} y {ydt}")


def test_colstat_split16_gives_the_integer_sums(dev, e=0):
    """The wide split kernel takes column statistics from T >= 128: (3, 128) only."""
    from speech_diarization_amd import ops
    c = E.conv_case("C3x128-256", e, "split")
    n_cs = ops.colstat_floats(c.M, c.cout)
    cs = torch.full((n_cs + 4096,), NAN, device=dev)
    with expect_launches(exactly=E.split_labels("C3x128-256"), family=SPLIT_CONV):
        got = run_conv(dev, c, "wide", colstat=cs)
    check_conv(dev, c, got, F32, "split16")
    _check_colstat(dev, c, got["y"], cs, n_cs, F32, "C3x128-256 split16")


@pytest.mark.parametrize("kind", ["onehot", "sums"])
@pytest.mark.parametrize("B,T,dil", E.CHAIN_SHAPES)
def test_res2net_chain_f16_gives_the_integer_chain(dev, kind, B, T, dil, e=0):
    """The fused chain must equal the integer chain, and the seven unfused f16 convs (tee + tee_add carrying c_{j+1} + y_j) must give
    the same bits.  "onehot": a composition of gathers and adds; "sums": four +-1 weights per output channel."""
    from speech_diarization_amd import ops
    n = 7
    assert ops.res2net_chain_supported(T, 128, n, 3, dil)
    r, layers, want = E.chain_case(kind, B, T, dil, e=e)
    dl = [dict(w=ops.pack_weight(L["w"], dev, F16), bias=_dev(L["bias"], F32, dev), scale=_dev(L["scale"], F32, dev),
               shift=_dev(L["shift"], F32, dev), dil=dil) for L in layers]
    got = _dev(r, F16, dev)
    with expect_launches(exactly=["chain_pack_kernel", f"res2net_chain_f16_kernel<{(T + 31) // 32}>"]):      # one instantiation per 32-row time tile
        ops.res2net_chain(got, T, dl)
        torch.cuda.synchronize()
    _same(got, _dev(want, F16, dev), f"chain {kind} T={T}")
    un = _dev(r, F16, dev)
    s0 = un[:, 128:256].clone()
    s1 = torch.empty_like(s0)
    with expect_launches(exactly=["conv_gemm_f16_kernel<f16,f16>"], family=F16_CONV):
        for j in range(1, n + 1):
            src, dst = (s0, s1) if j & 1 else (s1, s0)
            L = dl[j - 1]
            kw = dict(cin=128, dil=dil, bias=L["bias"], act="relu", scale=L["scale"], shift=L["shift"], out=un, o_col0=128 * j)
            if j < n:
                kw.update(tee=dst, tee_lo=0, tee_hi=128, tee_add=un, ta_col0=128 * (j + 1))
            ops.conv1d_cl(src, L["w"], T, **kw)
        torch.cuda.synchronize()
    _same(un, got, f"unfused chain {kind} T={T}")


# ------------------------------------------------------------------ 2. reductions (sd_pool.hip, sd_asp_fused.hip)

def _dt(N, dtype):
    return N.SD_DT_F16 if dtype == F16 else N.SD_DT_F32


def _t(dtype):
    """The storage type as the launch labels write it."""
    return "f16" if dtype == F16 else "f32"


def _check_stats(got, mean, std, Cc, what, dev, e=0):
    """mean bit for bit; std bit for bit where the variance is a perfect square, sqrt(eps) where it is 0 (a twin at 2^e, whose eps is
    1e-12 4^e: sqrt(eps) 2^e)."""
    _same(got[:, :Cc], _dev(mean, F32, dev), what + " mean")
    if std is None:
        return
    root = float(np.ldexp(E.SQRT_EPS, e))
    var0 = torch.from_numpy(std == root).to(dev)
    square = torch.from_numpy(~np.isnan(std) & (std != root)).to(dev)
    sd = got[:, Cc:]
    _same(sd[square], _dev(std, F32, dev)[square], what + " std (perfect squares)")
    if int(var0.sum()):
        torch.testing.assert_close(sd[var0], torch.full_like(sd[var0], float(np.ldexp(1e-6, e))), rtol=1e-6, atol=0.0)


# (B, T, C): 16 x 16 workgroups (grid.x * B < 256) and 64 x 4 ones; C = 100 is what the entry takes of "100 padded to a multiple of 4"
REDUCE_SHAPES = [(5, 64, 100), (40, 64, 3072), (5, 128, 100)]
# the workgroup shape sd_seg_mean_std takes: 16 x 16 while ceil(C / 256) B < 256 (the 64 x 4 grid would be small), 64 x 4 from there on (12 x 40)
REDUCE_FORM = {(5, 64, 100): "16x16", (40, 64, 3072): "64x4", (5, 128, 100): "16x16"}


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("B,T,C_", REDUCE_SHAPES)
def test_seg_mean_std_and_se_scale_residual_uniform(dev, dtype, B, T, C_, e=0):
    from speech_diarization_amd import ops
    N, lib = _lib()
    d = E.reduction_case(B, T, C_, f16=dtype == F16, e=e)
    xbuf, xv = _framed(d["x"].reshape(B * T, C_), dtype, dev)
    out = torch.full((B, 2 * C_ + 8), NAN, device=dev)
    with expect_launches(exactly=[f"seg_mean_std_kernel<{_t(dtype)},uniform,{REDUCE_FORM[B, T, C_]}>"]):
        N.check(lib.sd_seg_mean_std_dt(xbuf.data_ptr(), _dt(N, dtype), xbuf.stride(0), 8, B, T, C_, 1, C.c_float(d["eps"]), out.data_ptr(), _stream()),
                "sd_seg_mean_std_dt")
        torch.cuda.synchronize()
    assert bool(torch.isnan(out.view(-1)[B * 2 * C_:]).all())
    _check_stats(out.view(-1)[:B * 2 * C_].view(B, 2 * C_), d["mean"], d["std"], C_, f"seg_mean_std {dtype}", dev, e)
    if dtype == F32:
        _same(ops.seg_mean(xbuf, B, T, col0=8, C_=C_), _dev(d["mean"], F32, dev), "seg_mean")
        _check_stats(ops.seg_mean_std(xv.contiguous(), B, T, eps=d["eps"]), d["mean"], d["std"], C_, "seg_mean_std_f32", dev, e)
    if C_ % 8 == 0 or dtype == F32:
        rbuf, _ = _framed(d["res"].reshape(B * T, C_), dtype, dev)
        ybuf = torch.full((B * T, C_ + 16), NAN, dtype=dtype, device=dev)
        x = xv.contiguous()
        with expect_launches(exactly=[f"se_scale_residual_kernel<{_t(dtype)},uniform>"]):
            N.check(lib.sd_se_scale_residual_dt(x.data_ptr(), x.stride(0), _dev(d["gate"], F32, dev).data_ptr(), rbuf.data_ptr(), rbuf.stride(0), 8,
                                                ybuf.data_ptr(), ybuf.stride(0), 8, B, T, C_, _dt(N, dtype), _stream()), "sd_se_scale_residual_dt")
            torch.cuda.synchronize()
        _untouched(ybuf, 8, 8 + C_, "se_scale_residual")
        _same(ybuf[:, 8:8 + C_], _dev(d["y"].reshape(B * T, C_), dtype, dev), f"se_scale_residual {dtype}")


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("T,n", E.LENS)
def test_seg_mean_std_with_lens_ignores_the_padded_frames(dev, dtype, T, n, e=0):
    """rel_len = n / T with n a power of two; every padded frame holds 1e30 (f16: 65504), so a frame that leaks shows."""
    N, lib = _lib()
    B, C_ = 5, 100
    d = E.reduction_case(B, T, C_, lens=(n,), f16=dtype == F16, e=e)
    rel = torch.tensor([float(E.rel_len(T, m)) if m != T else 1.0 for m in d["n_live"]], device=dev)
    xbuf, _ = _framed(d["x_poisoned"].reshape(B * T, C_), dtype, dev)
    out = torch.full((B, 2 * C_), NAN, device=dev)
    with expect_launches(exactly=[f"seg_mean_std_kernel<{_t(dtype)},uniform,16x16>"]):      # B = 5, one channel block: the small grid
        N.check(lib.sd_seg_mean_std_lens_dt(xbuf.data_ptr(), _dt(N, dtype), xbuf.stride(0), 8, B, T, rel.data_ptr(), C_, 1, C.c_float(d["eps"]),
                                            out.data_ptr(), _stream()), "sd_seg_mean_std_lens_dt")
        torch.cuda.synchronize()
    _check_stats(out, d["mean"], d["std"], C_, f"seg_mean_std lens T={T} n={n} {dtype}", dev, e)


@pytest.mark.parametrize("dtype", [F32, F16])
def test_seg_mean_std_and_se_scale_residual_packed(dev, dtype, e=0):
    """Packed spans of 64, 128, 32, 64 and 16 rows (powers of two: exact means): the span map of the statistics and of the gate."""
    from speech_diarization_amd import ops
    spans = (64, 128, 32, 64, 16)
    C_ = 104
    parts = [E.reduction_case(1, L, C_, f16=dtype == F16, seed=i, e=e) for i, L in enumerate(spans)]
    x = _dev(np.concatenate([p["x"][0] for p in parts]), dtype, dev)
    res = _dev(np.concatenate([p["res"][0] for p in parts]), dtype, dev)
    gate = _dev(np.concatenate([p["gate"] for p in parts]), F32, dev)
    fs = np.concatenate([[0], np.cumsum(spans)]).astype(np.int32)
    with expect_launches(exactly=[f"seg_mean_std_kernel<{_t(dtype)},packed,64x4>"]):       # a packed map never takes 16 x 16
        got = ops.seg_mean_std_packed(x, fs, eps=parts[0]["eps"])
        torch.cuda.synchronize()
    _check_stats(got, np.concatenate([p["mean"] for p in parts]), np.concatenate([p["std"] for p in parts]), C_, f"packed seg_mean_std {dtype}", dev, e)
    with expect_launches(exactly=[f"se_scale_residual_kernel<{_t(dtype)},packed>"]):
        y = ops.se_scale_residual_packed(x, gate, res, fs)
        torch.cuda.synchronize()
    _same(y, _dev(np.concatenate([p["y"][0] for p in parts]), dtype, dev), f"packed se_scale_residual {dtype}")


POOL_FAMILY = {"asp_pool_kernel", "asp_pool_lds_kernel"}


def _pool_label(dtype, T, C_):
    """sd_asp_pool: the LDS-resident kernel when C is a multiple of its channel tile (32 f32 / 64 f16; 128 is, 100 is not) and a
    segment's tile fits 64 KB (T <= 247: 201 does, 256 and 257 do not), the streaming kernel otherwise."""
    staged = C_ == 128 and T in (57, 128, 131, 201)
    assert staged or C_ == 100 or T in (256, 257), (T, C_)
    return f"asp_pool_lds_kernel<{_t(dtype)}>" if staged else f"asp_pool_kernel<{_t(dtype)},uniform>"


def _asp_pool(dev, logit, h, dtype, B, T, C_, rel=None, eps=1e-12):
    N, lib = _lib()
    lg, hd = _dev(logit.reshape(B * T, C_), dtype, dev), _dev(h.reshape(B * T, C_), dtype, dev)
    out = torch.full((B, 2 * C_), NAN, device=dev)
    with expect_launches(exactly=[_pool_label(dtype, T, C_)], family={"asp_pool_kernel", "asp_pool_lds_kernel"}):
        N.check(lib.sd_asp_pool_lens_dt(lg.data_ptr(), C_, hd.data_ptr(), _dt(N, dtype), C_, B, T, None if rel is None else rel.data_ptr(), C_,
                                        C.c_float(eps), out.data_ptr(), _stream()), "sd_asp_pool_lens_dt")
        torch.cuda.synchronize()
    return out


# C = 128: the LDS-resident kernel up to T = 248, the streaming kernel above; C = 100 (no multiple of the 32 / 64-channel tile): streaming
POOL_SHAPES = [(3, 128, 128), (3, 256, 128), (3, 64, 100), (2, 201, 128), (2, 257, 128)]


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("B,T,C_", POOL_SHAPES)
def test_asp_pool_one_hot_logits_return_one_frame(dev, dtype, B, T, C_, e=0):
    """logit 0 at t*(b, c) and -200 elsewhere: the mean is h[b, t*, c] bit for bit, the std sqrt(eps); t* walks both sides of every
    row-phase, staging-pass and chunk boundary, the first and the last frame."""
    d = E.pool_onehot_case(B, T, C_, e=e, f16=bool(e) and dtype == F16)
    got = _asp_pool(dev, d["logit"], d["h"], dtype, B, T, C_, eps=d["eps"])
    _check_stats(got, d["mean"], np.full_like(d["mean"], d["sqrt_eps"]), C_, f"asp_pool one-hot T={T} C={C_} {dtype}", dev, e)
    if dtype == F32:
        from speech_diarization_amd import ops
        plain = ops.asp_pool(_dev(d["logit"].reshape(B * T, C_), F32, dev), _dev(d["h"].reshape(B * T, C_), F32, dev), B, T, eps=d["eps"])
        _same(plain, got, "sd_asp_pool_f32")


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("B,T,C_", [(3, 128, 128), (3, 256, 128), (3, 64, 100)])
def test_asp_pool_uniform_weights_give_the_exact_mean_and_std(dev, dtype, B, T, C_, e=0):
    d = E.pool_uniform_case(B, T, C_, e=e, f16=bool(e) and dtype == F16)
    got = _asp_pool(dev, d["logit"], d["h"], dtype, B, T, C_, eps=d["eps"])
    _check_stats(got, d["mean"], d["std"], C_, f"asp_pool uniform T={T} C={C_} {dtype}", dev, e)


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("T,n", E.LENS)
@pytest.mark.parametrize("C_", [128, 100])
def test_asp_pool_with_lens_ignores_the_padded_frames(dev, dtype, T, n, C_, e=0):
    """A +200 logit and a 1e30 value (f16: 65504) sit in every padded frame."""
    B = 3
    d = E.pool_onehot_case(B, T, C_, lens=(n, T, n), e=e, f16=bool(e) and dtype == F16)
    rel = torch.tensor([float(E.rel_len(T, m)) if m != T else 1.0 for m in d["n_live"]], device=dev)
    got = _asp_pool(dev, d["logit"], d["h"] if dtype == F32 else d["h_f16"], dtype, B, T, C_, rel, eps=d["eps"])
    _check_stats(got, d["mean"], np.full_like(d["mean"], d["sqrt_eps"]), C_, f"asp_pool lens T={T} n={n} {dtype}", dev, e)


@pytest.mark.parametrize("dtype", [F32, F16])
@pytest.mark.parametrize("T,n", E.LENS)
@pytest.mark.parametrize("C_", [128, 100])
def test_asp_pool_with_lens_uniform_weights_over_the_live_frames(dev, dtype, T, n, C_, e=0):
    """Equal logits over the n live frames (a power of two), the padded ones poisoned: the exact mean and std of the live frames."""
    B = 3
    d = E.pool_uniform_case(B, T, C_, n=n, e=e, f16=bool(e) and dtype == F16)
    rel = torch.full((B,), float(E.rel_len(T, n)), device=dev)
    got = _asp_pool(dev, d["logit"], d["h"] if dtype == F32 else d["h_f16"], dtype, B, T, C_, rel, eps=d["eps"])
    _check_stats(got, d["mean"], d["std"], C_, f"asp_pool lens uniform T={T} n={n} {dtype}", dev, e)


def test_asp_pool_packed_one_hot(dev, e=0, dtypes=(F32, F16)):
    from speech_diarization_amd import ops
    spans = (64, 257, 5, 128)
    C_ = 128
    parts = [E.pool_onehot_case(1, L, C_, seed=i, e=e, f16=bool(e) and dtypes == (F16,)) for i, L in enumerate(spans)]
    fs = np.concatenate([[0], np.cumsum(spans)]).astype(np.int32)
    for dtype in dtypes:
        with expect_launches(exactly=[f"asp_pool_kernel<{_t(dtype)},packed>"], family=POOL_FAMILY):     # a packed map always streams
            got = ops.asp_pool_packed(_dev(np.concatenate([p["logit"][0] for p in parts]), dtype, dev),
                                      _dev(np.concatenate([p["h"][0] for p in parts]), dtype, dev), fs, eps=parts[0]["eps"])
            torch.cuda.synchronize()
        mean = np.concatenate([p["mean"] for p in parts])
        _check_stats(got, mean, np.full_like(mean, parts[0]["sqrt_eps"]), C_, f"asp_pool packed {dtype}", dev, e)


def _attend(dev, mode, a1, wc, h, B, T, C_, rel=None, eps=1e-12):
    from speech_diarization_amd import ops
    N, lib = _lib()
    dtype = F16 if mode == "f16" else F32
    a1d = _dev(a1.reshape(B * T, -1), dtype, dev)
    wp = ops.pack_weight(wc[:, :, None], dev, dtype)
    hd = _dev(h.reshape(B * T, C_), dtype, dev)
    out = torch.full((B, 2 * C_), NAN, device=dev)
    dt = {"f32": N.SD_DT_F32, "f16": N.SD_DT_F16, "split16": N.SD_DT_SPLIT16}[mode]
    with expect_launches(exactly=[_fused_label(mode, T)], family={"asp_attend_pool_f32_kernel", "asp_attend_pool_f16_kernel"}):
        N.check(lib.sd_asp_attend_pool_lens_dt(a1d.data_ptr(), wp.data_ptr(), hd.data_ptr(), dt, C_, B, T, None if rel is None else rel.data_ptr(),
                                               C_, a1d.shape[1], C.c_float(eps), out.data_ptr(), _stream()), "sd_asp_attend_pool_lens_dt")
        torch.cuda.synchronize()
    return out


def _fused_label(mode, T):
    """The templates of sd_asp_attend_pool_scaled: f32 / split16 in 16-frame tiles x 4, 8, 13, 16 (T <= 64, 128, 208, 256), f16 in wave
    slots of 64 frames x 1 .. 4."""
    if mode == "f16":
        return f"asp_attend_pool_f16_kernel<{(T + 63) // 64}>"
    nt = next(n for n in (4, 8, 13, 16) if T <= 16 * n)
    return f"asp_attend_pool_f32_kernel<{nt}{',split' if mode == 'split16' else ''}>"


# T on both sides of every template of the fused kernels: f32 / split16 16-frame tiles x 4, 8, 13, 16; f16 wave slots x 1 .. 4
FUSED_T = [64, 65, 128, 129, 192, 193, 208, 209, 256]


@pytest.mark.parametrize("mode", ["f32", "f16", "split16"])
@pytest.mark.parametrize("T", FUSED_T)
def test_fused_attention_pooling_one_hot(dev, mode, T, e=0):
    """The logits are built inside the kernel from a one-hot a1 and an integer wc (0 at t*, -200 elsewhere)."""
    B, C_ = 3, 256
    d = E.pool_onehot_case(B, T, C_, fused=True, e=e, f16=bool(e) and mode == "f16")
    a1, wc = E.attend_factors(d["logit"])
    got = _attend(dev, mode, a1, wc, d["h"], B, T, C_, eps=d["eps"])
    _check_stats(got, d["mean"], np.full_like(d["mean"], d["sqrt_eps"]), C_, f"fused one-hot {mode} T={T}", dev, e)


@pytest.mark.parametrize("mode", ["f32", "f16", "split16"])
@pytest.mark.parametrize("T", [64, 128, 256])
def test_fused_attention_pooling_uniform_weights(dev, mode, T, e=0):
    """All logits 0 (see the module docstring for why not another level): the exact mean; the f32 / split16 kernels (two-pass variance)
    the exact std as well, the f16 kernel (E[h^2] - mu^2 in f32, exact on these integers) too."""
    B, C_ = 3, 256
    d = E.pool_uniform_case(B, T, C_, level=0.0, fused=True, e=e, f16=bool(e) and mode == "f16")
    a1, wc = E.attend_factors(d["logit"])
    got = _attend(dev, mode, a1, wc, d["h"], B, T, C_, eps=d["eps"])
    _check_stats(got, d["mean"], d["std"], C_, f"fused uniform {mode} T={T}", dev, e)


@pytest.mark.parametrize("mode", ["f32", "f16", "split16"])
@pytest.mark.parametrize("T,n", E.LENS)
def test_fused_attention_pooling_with_lens_ignores_the_padded_frames(dev, mode, T, n, e=0):
    B, C_ = 3, 256
    d = E.pool_onehot_case(B, T, C_, lens=(n, T, n), fused=True, e=e, f16=bool(e) and mode == "f16")
    a1, wc = E.attend_factors(d["logit"])
    rel = torch.tensor([float(E.rel_len(T, m)) if m != T else 1.0 for m in d["n_live"]], device=dev)
    got = _attend(dev, mode, a1, wc, d["h_f16"] if mode == "f16" else d["h"], B, T, C_, rel, eps=d["eps"])
    _check_stats(got, d["mean"], np.full_like(d["mean"], d["sqrt_eps"]), C_, f"fused lens {mode} T={T} n={n}", dev, e)


@pytest.mark.parametrize("mode", ["f32", "f16", "split16"])
@pytest.mark.parametrize("T,n", E.LENS)
def test_fused_attention_pooling_with_lens_uniform_weights_over_the_live_frames(dev, mode, T, n, e=0):
    """Logits 0 over the n live frames, a +200 logit and 1e30 (f16: 65504) in every padded one: the exact mean and std of the live
    frames.  (The one-hot case cannot see a padded value that reaches the variance: its expected std is the clamp itself.)"""
    B, C_ = 3, 256
    d = E.pool_uniform_case(B, T, C_, level=0.0, fused=True, n=n, e=e, f16=bool(e) and mode == "f16")
    a1, wc = E.attend_factors(d["logit"])
    rel = torch.full((B,), float(E.rel_len(T, n)), device=dev)
    got = _attend(dev, mode, a1, wc, d["h_f16"] if mode == "f16" else d["h"], B, T, C_, rel, eps=d["eps"])
    _check_stats(got, d["mean"], d["std"], C_, f"fused lens uniform {mode} T={T} n={n}", dev, e)


# ------------------------------------------------------------------ 3. products outside the network

def _affinity_labels(n, split16, whole, aligned):
    """ops.cosine_affinity: the triangle kernel for the whole matrix when N % 4 == 0 and the output takes 16-byte stores; otherwise
    the conv operators -- f32: the symmetric launch (whole matrix) or a plain one (`rows=`), which the 32x32 split-K kernel takes
    below 128 tiles of 128x128 (N <= 1408) and the band walk of the 128x128 kernel above; split16: a filled 2^-8 scale and the wide
    split conv, whose epilogue is the staged one on these slices (N % 8 != 0 or an odd ldo)."""
    helpers = ["l2norm_rows_kernel"] + (["split16_pack_kernel"] if split16 else [])
    if whole and aligned and n % 4 == 0:
        return helpers + ["affinity_sym_kernel<split16x3>" if split16 else "affinity_sym_kernel<exact f32>"]
    if split16:
        return helpers + ["fill_f32_kernel", "conv_gemm_f16_t256_kernel<split,staged>/grid"]
    return helpers + ["conv_gemm_f32_kernel<dma>/symmetric" if whole and (-(-n // 128)) ** 2 >= 128 else "skinny_gemm_f32_kernel"]


AFFINITY_FAMILY = F32_CONV | SPLIT_CONV | {"affinity_sym_kernel"}


@pytest.mark.parametrize("n", [4, 132, 260, 1030, 1412])
def test_cosine_affinity_is_k_over_16(dev, n, e=0):
    """f32 and split16 (its alpha is 2^-8 and its row scale 2^4: powers of two, so the whole-matrix path is exact and stays in), the whole
    matrix and `rows=` blocks, a tight and a padded output (an odd ldo takes the paths without 16-byte stores).  n = 1412 = 12 tiles
    of 128: the smallest multiple of 4 whose unaligned whole matrix leaves the split-K kernel for the symmetric band walk of the
    128x128 kernel (12 x 12 = 144 >= 128 tiles)."""
    from speech_diarization_amd import ops
    X, K = E.affinity_rows(n, e=e)
    xd = _dev(X, F32, dev)
    want = _dev(K, F32, dev)
    for split16 in (False, True):
        for pad in (0, 4, 7):
            buf = torch.full((n, n + pad), NAN, device=dev)
            with expect_launches(exactly=_affinity_labels(n, split16, True, pad != 7), family=AFFINITY_FAMILY):
                ops.cosine_affinity(xd, out=buf[:, :n] if pad else buf, split16=split16)
                torch.cuda.synchronize()
            _untouched(buf, 0, n, "cosine_affinity")
            got = buf[:, :n]
            _same(got, want, f"cosine_affinity n={n} split16={split16} pad={pad}")
            assert torch.equal(got, got.T) and bool((got[2] == 0).all()) and bool((got[:, 2] == 0).all())
            assert got[0, 1] == 1 and got[0, n - 1] == 1 and got[n - 1, 1] == 1
        for lo, hi in ((0, min(n, 3)), (n // 3, n // 3 + min(n - n // 3, 130)), (n - 1, n)):
            with expect_launches(exactly=_affinity_labels(n, split16, False, True), family=AFFINITY_FAMILY):
                blk = ops.cosine_affinity(xd, rows=(lo, hi), split16=split16)
                torch.cuda.synchronize()
            _same(blk, want[lo:hi], f"cosine_affinity rows [{lo}, {hi}) n={n} split16={split16}")


@pytest.mark.parametrize("n", [129, 257, 300])
@pytest.mark.parametrize("d", [7, 190, 192])
def test_ahc_nearest_breaks_every_tie_towards_the_lowest_index(dev, n, d):
    from speech_diarization_amd import ops
    for ld in ((d + 3) // 4 * 4, (d + 3) // 4 * 4 + 8):
        S, count, inv, nn_want, best_want = E.ahc_case(n, d, ld)
        sums = _dev(S, F32, dev)[:, :d] if ld > d else _dev(S, F32, dev)
        inv_d = _dev(inv, F32, dev)
        with expect_launches(exactly=["ahc_nearest_kernel", "ahc_nearest_finish_kernel"]):
            nn, best = ops.ahc_nearest(sums, inv_d)
            torch.cuda.synchronize()
        _same(nn, torch.from_numpy(nn_want).to(dev), f"ahc nn n={n} d={d} ld={ld}")
        _same(best, _dev(best_want, F32, dev), f"ahc best n={n} d={d} ld={ld}")
        nn_h = nn.cpu().numpy()
        pairs = np.nonzero(nn_h[nn_h] == np.arange(n))[0]
        assert pairs.size >= 2 and torch.equal(best[pairs], best[nn_h[pairs]])         # reciprocal pairs carry equal bits
        cnt = _dev(count, F32, dev)
        s_ref, c_ref, i_ref, t_ref, m_ref = ahc_ref.merge_f32(np.nan_to_num(S[:, :d]), count, inv, nn_h, best.cpu().numpy(), 0.0)
        with expect_launches(exactly=["ahc_merge_kernel"]):
            target, n_merged = ops.ahc_merge(sums, cnt, inv_d, nn, best, 0.0)
            torch.cuda.synchronize()
        assert int(n_merged) == m_ref and m_ref >= 1
        _same(target, torch.from_numpy(t_ref).to(dev), "ahc merge target")
        _same(sums.contiguous(), torch.from_numpy(s_ref).to(dev), "ahc merged sums")
        _same(cnt, torch.from_numpy(c_ref).to(dev), "ahc merged counts")
        _same(inv_d, torch.from_numpy(i_ref).to(dev), "ahc merged inv_count")


@pytest.mark.parametrize("n", [129, 600, 1030])
@pytest.mark.parametrize("b", [8, 16, 24, 32])
def test_affinity_apply_and_degree_are_exact(dev, n, b):
    """n = 600 and 1030 split the columns over 2 and 3 workgroups; an aligned ld (16-byte loads) and an odd one (scalar loads); a dyadic
    case and a one-hot V whose answer names the entry of K that was read."""
    from speech_diarization_amd import ops
    for ld in ((n + 3) // 4 * 4 + 4, n + 3 if (n + 3) % 4 else n + 5):
        for onehot in (False, True):
            K, scale, V = E.spectral_case(n, b, ld, onehot=onehot)
            Kd = _dev(K, F32, dev)[:, :n]
            for zero_diag in (False, True):
                deg, Y = E.spectral_expected(K, scale, V, zero_diag)
                what = f"n={n} b={b} ld={ld} onehot={onehot} zero_diag={zero_diag}"
                with expect_launches(exactly=["affinity_degree_kernel"]):
                    got_deg = ops.affinity_degree(Kd, zero_diag)
                # <blocks of 16 columns per thread, loads of K>: the aligned ld takes the 16-byte loads, the odd one the scalar loads
                with expect_launches(exactly=[f"affinity_apply_kernel<{1 if b <= 16 else 2},{'vec' if ld % 4 == 0 else 'scalar'}>", "apply_finish_kernel"]):
                    got_y = ops.affinity_apply(Kd, _dev(scale, F32, dev), _dev(V, F32, dev), zero_diag)
                _same(got_deg, _dev(deg, F32, dev), "affinity_degree " + what)
                _same(got_y, _dev(Y, F32, dev), "affinity_apply " + what)


@pytest.mark.parametrize("K", [1, 5, 64])
@pytest.mark.parametrize("N_", [1, 41, 130])
@pytest.mark.parametrize("D", [7, 192, 200])
def test_sim_argmax_returns_the_first_maximum(dev, K, N_, D, e=0):
    from speech_diarization_amd import ops
    w, c, best_want, score_want = E.argmax_case(N_, K, D, e=e)
    with expect_launches(exactly=["sim_argmax_kernel"]):
        best, score = ops.sim_argmax(_dev(w, F32, dev), _dev(c, F32, dev))
        torch.cuda.synchronize()
    _same(best, torch.from_numpy(best_want).to(dev), f"sim_argmax best K={K} N={N_} D={D}")
    _same(score, _dev(score_want, F32, dev), f"sim_argmax score K={K} N={N_} D={D}")


def test_adjacent_cosine_and_l2norm_rows_are_exact(dev, e=0):
    """Rows of norm 4 with eps = 0 / eps_add = 0; a zero row under the sklearn guard."""
    from speech_diarization_amd import ops
    X, K = E.affinity_rows(133, e=e)
    live = np.delete(X, 2, axis=0)                        # without the zero row: 0 / 0 has no exact answer
    X, live = E.scaled(-e, X, live)                       # (the expected values below: those of the unscaled rows)
    Kl = (live @ live.T) / 16.0
    with expect_launches(exactly=["adjacent_cosine_kernel"]):
        adj = ops.adjacent_cosine(_dev(E.scaled(e, live), F32, dev), eps=0.0)
    _same(adj, _dev(np.diagonal(Kl, 1).copy(), F32, dev), "adjacent_cosine")
    with expect_launches(exactly=["l2norm_rows_kernel"]):
        unit = ops.l2norm_rows(_dev(E.scaled(e, live), F32, dev))
    _same(unit, _dev(live / 4.0, F32, dev), "l2norm_rows")
    _same(ops.l2norm_rows(_dev(E.scaled(e, X), F32, dev), sklearn_zero_guard=True), _dev(X / 4.0, F32, dev), "l2norm_rows (sklearn guard)")


@pytest.mark.parametrize("n", [50, 257, 1000])
@pytest.mark.parametrize("k", [1, 64, "n"])
def test_topk_mean_std_on_tied_integer_rows(dev, n, k, e=0):
    """The k-th value tied many times, mixed signs (the ordered-key map flips at 0), +0.0 and -0.0 together, ld > n."""
    from speech_diarization_amd import ops
    k = n if k == "n" else k
    x, mean, std = E.topk_case(n, k, e=e)
    buf = torch.full((x.shape[0], n + 5), NAN, device=dev)
    buf[:, :n] = torch.from_numpy(x).to(dev)               # (float64 -> f32 keeps the sign of -0.0)
    with expect_launches(exactly=["topk_mean_std_kernel"]):
        got = ops.topk_mean_std(buf[:, :n], k)
        torch.cuda.synchronize()
    ok_m, ok_s = torch.from_numpy(~np.isnan(mean)).to(dev), torch.from_numpy(~np.isnan(std)).to(dev)
    assert int(ok_m.sum()) >= (7 if min(k, n) & (min(k, n) - 1) == 0 else 1)
    _same(got[:, 0][ok_m], _dev(mean, F32, dev)[ok_m], f"topk mean n={n} k={k}")
    _same(got[:, 1][ok_s], _dev(std, F32, dev)[ok_s], f"topk std n={n} k={k}")


@pytest.mark.parametrize("K", [2, 8, 64])
@pytest.mark.parametrize("T", [1, 2, 128, 129, 130, 257])
def test_viterbi_ties_go_to_the_first_state(dev, K, T):
    """The chunk edges of VT_CHUNK = 128 on the forward pass and the backtrack; alpha < 1 / K makes moving beat staying, so all i != j
    candidates tie and the first must win."""
    from speech_diarization_amd import diar_diag, ops
    s = E.viterbi_scores(T, K)
    for alpha in (0.9, 0.995, 0.01):
        want = diar_diag.viterbi_hmm(s, alpha)
        with expect_launches(exactly=["viterbi_kernel"]):
            got = ops.viterbi(torch.from_numpy(s).to(dev), alpha)
            torch.cuda.synchronize()
        _same(got, torch.from_numpy(want).to(dev), f"viterbi K={K} T={T} alpha={alpha}")
