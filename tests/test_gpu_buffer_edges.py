"""No entry of libsd_hip.so reads or writes outside the buffers it is handed.

include/sd_hip.h promises that the library never allocates: the caller owns every byte, asks a sizing function how much scratch an
entry needs and hands over exactly that.  Here every exported entry that takes a device pointer runs through the raw C ABI with
  * every input, output, table and workspace in a guarded buffer of EXACTLY the documented size (tests/helpers/guarded.py: 4 MiB of
    0xFF in front of and behind the payload; 0xFF.. is a NaN as f32 and f16 and -1 as an index),
  * inputs as slices that end where their buffer ends (a K step or a 16-byte load past the slice reads NaN), outputs as column
    slices in the middle of a wider poisoned matrix (the neighbours must keep their bytes),
  * outputs and workspace pre-filled with each of three poisons (0xFF, 0x7B, 0x00).
Per case: all guards intact, neighbours unchanged, results finite, BITWISE equal under the three poisons (the entries are bitwise
repeatable run to run, so a difference between two poisons means stale or foreign bytes reached a result), and within the operator's
existing bar of its float64 reference (bars and reference code are those of the operator's own test module).

CASES maps an entry name to its guarded cases; tests/test_buffer_rules.py (no GPU) reads the entry names from the header and fails
for one that is neither a key of CASES nor exempted there with a reason."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import captured as CAP  # noqa: E402
import guarded as G  # noqa: E402
from kernel_selection import CONV_KERNELS, restore_conv_kernel, select_conv_kernel  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F16, I32, I64, U8 = torch.float32, torch.float16, torch.int32, torch.int64, torch.uint8
SD_ERR_WORKSPACE = -3
BAR = {"f32": 1e-5, "f32ns": 1e-5, "f32s": 1e-5, "f16": 1e-3}          # cosine distance to the float64 oracle, as in the suite
TILE_ROWS = (32, 64, 80, 96, 112, 128, 256)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _arg(a):
    if isinstance(a, G.Guarded):
        return a.ptr
    if isinstance(a, torch.Tensor):
        return a.data_ptr()
    return a


def call(name, *args):
    """The raw entry on the current stream -> its status (eagerly, or captured and replayed inside tests/helpers/captured.py's scopes)."""
    return CAP.call(name, *args)


def ok(name, *args):
    N.check(call(name, *args), name)


def _cos_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def _bits(t):
    return t.contiguous().view(-1).view(U8)


class Arena:
    """The guarded buffers of ONE call under ONE poison."""

    def __init__(self, dev, poison):
        self.dev, self.poison, self.bufs, self.slices = dev, poison, [], []

    def _new(self, nbytes, fill, name):
        g = G.guarded(nbytes, fill, self.dev, name)
        self.bufs.append(g)
        return g

    def data(self, t, name):
        """An input of exactly t's bytes: its last element is the payload's last."""
        return self._new(t.numel() * t.element_size(), 0, name).put(t)

    def scratch(self, nbytes, name):
        return self._new(int(nbytes), self.poison, name)

    def right(self, x, ld, name):
        """x [M, c] as the right-hand column slice of a [M, ld] matrix whose other columns are 0xFF -> (buffer, col0)."""
        M, c = x.shape
        g = self._new(M * ld * x.element_size(), 0xFF, name)
        g.view(x.dtype, M, ld)[:, ld - c:] = x.to(self.dev)
        return g, ld - c

    def cut(self, x, ld, name):
        """x [M, c] as rows of stride ld starting at the payload's first byte, the last row cut after its c values (the gaps 0xFF):
        for entries that take a row stride but no column offset."""
        M, c = x.shape
        g = self._new(((M - 1) * ld + c) * x.element_size(), 0xFF, name)
        flat = g.view(x.dtype)
        torch.as_strided(flat, (M, c), (ld, 1)).copy_(x.to(self.dev))
        return g

    def out(self, rows, cols, ld, col0, dtype, name):
        """A poisoned [rows, ld] matrix of which an entry may write columns [col0, col0 + cols) -> (buffer, that slice)."""
        g = self._new(rows * ld * torch.empty((), dtype=dtype).element_size(), self.poison, name)
        m = g.view(dtype, rows, ld)
        self.slices.append((m, col0, col0 + cols, name))
        return g, m[:, col0:col0 + cols]

    def out_cut(self, rows, cols, ld, dtype, name):
        """A poisoned output of rows of stride ld, the last one cut after `cols` values -> (buffer, strided view [rows, cols])."""
        es = torch.empty((), dtype=dtype).element_size()
        g = self._new(((rows - 1) * ld + cols) * es, self.poison, name)
        flat = g.view(dtype)
        v = torch.as_strided(flat, (rows, cols), (ld, 1))
        if ld > cols and rows > 1:
            gaps = torch.as_strided(flat, (rows - 1, ld - cols), (ld, 1), flat.storage_offset() + cols)
            self.slices.append((gaps, 0, 0, name + " (gap columns)"))
        return g, v

    def check(self):
        torch.cuda.synchronize()
        try:
            G.assert_guards_intact(*self.bufs)
        except G.GuardError as e:
            # a stray write: the state of device memory is unknown from here on, so nothing more runs on the GPU in this session
            pytest.exit(f"guard band overrun, stopping the session: {e}", returncode=1)
        for m, lo, hi, name in self.slices:
            G.assert_columns_keep(m, lo, hi, self.poison, name)


def under_poisons(dev, case, finite=True):
    """case(arena) -> {name: result tensor}; run under the three poisons, checked for guards, neighbours, finiteness and bitwise
    equality; -> the results of the first run (on the CPU)."""
    runs = []
    for p in G.POISONS:
        A = Arena(dev, p)
        res = case(A)
        A.check()
        res = {k: v.detach().clone().cpu() for k, v in res.items()}
        for k, v in res.items():
            if finite and v.is_floating_point():
                assert bool(torch.isfinite(v.float()).all()), f"poison 0x{p:02X}: {k} is not finite ({int((~torch.isfinite(v.float())).sum())} values)"
        runs.append(res)
        del A
    for p, r in zip(G.POISONS[1:], runs[1:]):
        for k in runs[0]:
            same = _bits(runs[0][k]) == _bits(r[k])
            if not bool(same.all()):
                i = int(torch.nonzero(~same)[0, 0]) // runs[0][k].element_size()
                raise AssertionError(f"{k}: poison 0x{p:02X} changed the result (first at flat element {i} of {tuple(r[k].shape)}): "
                                     f"{runs[0][k].view(-1)[i].item()} under 0xFF, {r[k].view(-1)[i].item()} under 0x{p:02X}")
    return runs[0]


@contextlib.contextmanager
def selection(entry, sel):
    """`sel` pinned process-wide for the duration: one of CONV_KERNELS for the exact-f32 operator (and the f32 forwards), "wide256" /
    "auto" for sd_conv1d_cl_f16 (the `f16_tiles` of tests/test_gpu_short_segments.py); None: the shipped rules."""
    lib = N.load()
    if entry == "sd_conv1d_cl_f16":
        N.check(lib.sd_set_tuning(N.SD_TUNE_F16_NARROW_TILES, 0 if sel == "wide256" else -1), "sd_set_tuning")
    elif sel:
        select_conv_kernel(sel)
    try:
        yield
    finally:
        restore_conv_kernel()
        N.check(lib.sd_set_tuning(N.SD_TUNE_F16_NARROW_TILES, -1), "sd_set_tuning")


CASES = {}


def case(entry, cid):
    def deco(fn):
        CASES.setdefault(entry, []).append((cid, fn))
        return fn
    return deco


def add(entry, cid, fn):
    CASES.setdefault(entry, []).append((cid, fn))


# ====================================================================== 3. operators

def _ref_conv_cl(x, w, b, T, dil):
    """x [M, cin] channel-last, w [cout, cin, k]; 'same' reflect conv per segment (float64)."""
    M, cin = x.shape
    xt = x.view(M // T, T, cin).transpose(1, 2)
    pad = dil * (w.shape[2] - 1) // 2
    if pad:
        xt = F.pad(xt, (pad, pad), mode="reflect")
    return F.conv1d(xt, w, b, dilation=dil).transpose(1, 2).reshape(M, -1)


def _ref_conv_spans(x, w, b, T_list, dil):
    out, r = [], 0
    pad = dil * (w.shape[2] - 1) // 2
    for T in T_list:
        xt = x[r:r + T].t()[None]
        if pad:
            xt = F.pad(xt, (pad, pad), mode="reflect")
        out.append(F.conv1d(xt, w, b, dilation=dil)[0].t())
        r += T
    return torch.cat(out)


def _conv_data(seed, M, cin, cout, k, B):
    g = torch.Generator().manual_seed(seed)
    d = dict(x=torch.randn(M, cin, generator=g, dtype=torch.float64),
             w=torch.randn(cout, cin, k, generator=g, dtype=torch.float64) / np.sqrt(cin * k),
             b=torch.randn(cout, generator=g, dtype=torch.float64),
             scale=torch.rand(cout, generator=g, dtype=torch.float64) + 0.5,
             shift=torch.randn(cout, generator=g, dtype=torch.float64),
             segb=torch.randn(B, cout, generator=g, dtype=torch.float64),
             add=torch.randn(M, cout, generator=g, dtype=torch.float64))
    return d


def _args(**kw):
    a = N.sd_conv_args()
    for k, v in kw.items():
        setattr(a, k, _arg(v))
    return a


_ACT = dict(none=N.SD_ACT_NONE, relu=N.SD_ACT_RELU, tanh=N.SD_ACT_TANH, sigmoid=N.SD_ACT_SIGMOID)
_ES = {F32: 4, F16: 2}
_DT = {F32: N.SD_DT_F32, F16: N.SD_DT_F16}

# (B, T, cin, cout, k, dil): M = B * T a multiple of no tile height, or one tile + 1 row; cin not a multiple of the K step;
# cout not a tile multiple / not a multiple of 8 (scalar epilogue); dilated taps
CONV_SHAPES = [
    (7, 19, 80, 192, 5, 1),        # M = 133, the stem's cin (80 -> cin_pad 96 / 128)
    (3, 43, 1000, 36, 3, 2),       # M = 129 = one 128-row tile + 1 row; K = 1000 (cin_pad 1024)
    (1, 257, 80, 1100, 3, 4),      # M = 257 = one 256-row tile + 1 row; wide output, cout % 8 != 0
    (11, 13, 1000, 192, 3, 4),     # M = 143
]


def test_conv_shapes_meet_no_tile_height_or_overhang_by_one_row():
    for B, T, *_ in CONV_SHAPES:
        M = B * T
        assert all(M % h for h in TILE_ROWS) and (any(M % h == 1 for h in TILE_ROWS) or M % 2 == 1), (B, T)
    assert 129 % 128 == 1 and 257 % 256 == 1


def _conv_plain(entry, sel, shape, xdt=F32, ydt=F32, o_shift=0):
    """bias + relu + affine, x as the right-hand slice of a wider matrix, y in the middle of a wider poisoned one.  o_shift: moves the
    output slice off its 16-byte alignment (the entry must take its scalar epilogue)."""
    B, T, cin, cout, k, dil = shape
    M = B * T
    half = entry == "sd_conv1d_cl_f16"

    def run(dev):
        from speech_diarization_amd import ops
        d = _conv_data(M * 7 + cout + cin, M, cin, cout, k, B)
        xq = d["x"].to(xdt)
        wq = d["w"].half() if half else d["w"].float()
        ref = torch.relu(_ref_conv_cl(xq.double(), wq.double(), d["b"], T, dil)) * d["scale"] + d["shift"]
        wp = ops.pack_weight(d["w"].float(), dev, F16 if half else F32)
        al = 8 if half else 4
        lda = cin + 6 * al
        gran = 8 if half else 4
        ldo, o_col0 = cout + 5 * gran + o_shift, 2 * gran + o_shift

        def one(A):
            x, a_col0 = A.right(xq, lda, "x")
            w = A.data(wp, "w")
            bias, scale, shift = A.data(d["b"].float(), "bias"), A.data(d["scale"].float(), "scale"), A.data(d["shift"].float(), "shift")
            y, yv = A.out(M, cout, ldo, o_col0, ydt, "y")
            a = _args(x=x, lda=lda, a_col0=a_col0, x_dtype=_DT[xdt], w=w, w_dtype=_DT[F16 if half else F32], y=y, ldo=ldo, o_col0=o_col0,
                      y_dtype=_DT[ydt], M=M, T=T, cin=cin, cin_pad=wp.shape[2], cout=cout, taps=k, dil=dil, bias=bias, act=_ACT["relu"],
                      scale=scale, shift=shift)
            ok(entry, C.byref(a))
            return {"y": yv}
        with selection(entry, sel):
            got = under_poisons(dev, one)["y"]
        err = (got.double() - ref).abs().max().item()
        tol = (1e-3 if ydt == F16 else 2e-5) * max(1.0, ref.abs().max().item())       # test_conv1d_cl_matches_torch / test_short_conv1d_cl_f16_matches_f64
        assert err < tol, (err, tol)
    return run


def _conv_epilogues(entry, sel, B, T, cin, cout, dil, dt=F32, with_add=True):
    """per-segment bias (table of exactly B x cout), act2, tee (+ tee_add: the 128x128 kernels; the 256x256 ones carry the store-only
    tee): every operand a slice that ends where its buffer ends, y and tee in the middle of wider poisoned matrices."""
    M = B * T
    half = entry == "sd_conv1d_cl_f16"

    def run(dev):
        from speech_diarization_amd import ops
        d = _conv_data(M + cout, M, cin, cout, 3, B)
        xq, addq = d["x"].to(dt), d["add"].to(dt)
        wq = d["w"].half() if half else d["w"].float()
        y_ref = _ref_conv_cl(xq.double(), wq.double(), None, T, dil) + d["segb"].float().double().repeat_interleave(T, dim=0)
        y_ref = torch.sigmoid(torch.relu(y_ref) * d["scale"].float().double() + d["shift"].float().double())
        wp = ops.pack_weight(d["w"].float(), dev, F16 if half else F32)
        g = 8
        lda, ldo, o_col0, ldt, t_col0, ld_ta = cin + 3 * g, cout + 4 * g, g, cout + 5 * g, 2 * g, cout + 2 * g

        def one(A):
            x, a_col0 = A.right(xq, lda, "x")
            w = A.data(wp, "w")
            segb, scale, shift = A.data(d["segb"].float(), "segb"), A.data(d["scale"].float(), "scale"), A.data(d["shift"].float(), "shift")
            if with_add:
                ta, ta_col0 = A.right(addq, ld_ta, "tee_add")
            y, yv = A.out(M, cout, ldo, o_col0, dt, "y")
            tee, tv = A.out(M, cout, ldt, t_col0, dt, "tee")
            a = _args(x=x, lda=lda, a_col0=a_col0, x_dtype=_DT[dt], w=w, w_dtype=_DT[F16 if half else F32], y=y, ldo=ldo, o_col0=o_col0,
                      y_dtype=_DT[dt], M=M, T=T, cin=cin, cin_pad=wp.shape[2], cout=cout, taps=3, dil=dil, bias=segb, bias_per_seg=1,
                      act=_ACT["relu"], scale=scale, shift=shift, act2=_ACT["sigmoid"], tee=tee.ptr + t_col0 * _ES[dt], ldt=ldt, tee_lo=0,
                      tee_hi=cout)
            if with_add:
                a.tee_add, a.ld_ta, a.ta_col0 = ta.ptr, ld_ta, ta_col0
            ok(entry, C.byref(a))
            return {"y": yv, "tee": tv}
        with selection(entry, sel):
            got = under_poisons(dev, one)
        bar = 1e-3 if half else 1e-5                  # test_short_conv1d_cl_f32_epilogues / test_short_conv1d_cl_f16_staged_epilogue
        assert (got["y"].double() - y_ref).abs().max() < bar
        if with_add:                                  # f16: test_conv1d_cl_f16_tee
            assert (got["tee"].double() - (y_ref + addq.double())).abs().max() < (4e-3 if half else 1e-5)
        else:
            assert torch.equal(got["tee"], got["y"])
    return run


def _conv_colstat(entry, sel, B, T, cin, cout, dt=F32):
    """colstat of exactly sd_colstat_floats, then sd_colstat_finish_dt on it."""
    M = B * T
    half = entry == "sd_conv1d_cl_f16"

    def run(dev):
        from speech_diarization_amd import ops
        d = _conv_data(T * 7 + cout, M, cin, cout, 1, B)
        xq = d["x"].to(dt)
        wp = ops.pack_weight(d["w"].float(), dev, F16 if half else F32)
        n_cs = int(N.load().sd_colstat_floats(M, cout))
        lda, ldo, o_col0 = cin + 16, cout + 24, 8

        def one(A):
            x, a_col0 = A.right(xq, lda, "x")
            w = A.data(wp, "w")
            bias, scale, shift = A.data(d["b"].float(), "bias"), A.data(d["scale"].float(), "scale"), A.data(d["shift"].float(), "shift")
            y, yv = A.out(M, cout, ldo, o_col0, dt, "y")
            cs = A.scratch(n_cs * 4, "colstat")
            a = _args(x=x, lda=lda, a_col0=a_col0, x_dtype=_DT[dt], w=w, w_dtype=_DT[F16 if half else F32], y=y, ldo=ldo, o_col0=o_col0,
                      y_dtype=_DT[dt], M=M, T=T, cin=cin, cin_pad=wp.shape[2], cout=cout, taps=1, dil=1, bias=bias, act=_ACT["relu"],
                      scale=scale, shift=shift, colstat=cs)
            ok(entry, C.byref(a))
            st = A.scratch(B * 2 * cout * 4, "stats")
            ok("sd_colstat_finish_dt", cs, shift, y, _DT[dt], ldo, o_col0, B, T, cout, 1, 1e-12, st)
            mean = A.scratch(B * cout * 4, "mean")
            ok("sd_colstat_finish_dt", cs, shift, y, _DT[dt], ldo, o_col0, B, T, cout, 0, 0.0, mean)
            return {"y": yv, "stats": st.view(F32, B, 2 * cout), "mean": mean.view(F32, B, cout)}
        with selection(entry, sel):
            got = under_poisons(dev, one)
        yr = got["y"].double().view(B, T, cout)
        tol = 2e-5 if dt == F32 else 2e-3                                    # test_epilogue_column_statistics
        assert (got["stats"][:, :cout].double() - yr.mean(1)).abs().max() < tol
        assert (got["stats"][:, cout:].double() - yr.std(1, unbiased=False)).abs().max() < tol
        assert torch.equal(got["mean"], got["stats"][:, :cout])
    return run


for _sel in CONV_KERNELS:
    for _i, _sh in enumerate(CONV_SHAPES):
        add("sd_conv1d_cl_f32", f"plain-{_sel}-{_i}", _conv_plain("sd_conv1d_cl_f32", _sel, _sh))
    add("sd_conv1d_cl_f32", f"unaligned-out-{_sel}", _conv_plain("sd_conv1d_cl_f32", _sel, (3, 43, 80, 36, 3, 2), o_shift=2))
    add("sd_conv1d_cl_f32", f"epilogues-{_sel}", _conv_epilogues("sd_conv1d_cl_f32", _sel, 9, 15, 128, 128, 4))
    add("sd_conv1d_cl_f32", f"colstat-{_sel}", _conv_colstat("sd_conv1d_cl_f32", _sel, 5, 65, 64, 256))
    add("sd_colstat_finish_dt", f"f32-{_sel}", _conv_colstat("sd_conv1d_cl_f32", _sel, 3, 129, 32, 512))
for _sel in ("wide256", "auto"):
    for _i, _sh in enumerate(CONV_SHAPES):
        _xdt = F32 if _sh[2] == 80 and _i == 0 else F16                    # the stem reads the f32 features
        add("sd_conv1d_cl_f16", f"plain-{_sel}-{_i}", _conv_plain("sd_conv1d_cl_f16", _sel, _sh, xdt=_xdt, ydt=F16))
    add("sd_conv1d_cl_f16", f"unaligned-out-{_sel}", _conv_plain("sd_conv1d_cl_f16", _sel, (3, 43, 80, 36, 3, 2), xdt=F16, ydt=F16, o_shift=4))
    add("sd_conv1d_cl_f16", f"f32-out-{_sel}", _conv_plain("sd_conv1d_cl_f16", _sel, (1, 257, 80, 1100, 3, 4), xdt=F16, ydt=F32))
    add("sd_conv1d_cl_f16", f"epilogues-{_sel}", _conv_epilogues("sd_conv1d_cl_f16", _sel, 9, 15, 128, 128, 4, dt=F16))
    add("sd_conv1d_cl_f16", f"epilogues-wide-{_sel}", _conv_epilogues("sd_conv1d_cl_f16", _sel, 9, 15, 128, 1032, 2, dt=F16, with_add=False))
    add("sd_conv1d_cl_f16", f"colstat-{_sel}", _conv_colstat("sd_conv1d_cl_f16", _sel, 3, 150, 64, 1024, dt=F16))
add("sd_colstat_finish_dt", "f16", _conv_colstat("sd_conv1d_cl_f16", "auto", 5, 201, 64, 256, dt=F16))


def _split_rows(x, cp):
    """f32 [M, c] -> SD_DT_SPLIT16 rows as f16 [M, 2 cp] (per 32 values [hi x 32 | lo x 32], zero padding), on the host."""
    M, c = x.shape
    v = torch.zeros(M, cp)
    v[:, :c] = x.float()
    hi = v.half()
    lo = (v - hi.float()).half()
    return torch.cat([hi.view(M, cp // 32, 32), lo.view(M, cp // 32, 32)], dim=2).reshape(M, 2 * cp)


def _conv_split16(shape, narrow, out_split=False, epilogues=False):
    B, T, cin, cout, k, dil = shape
    M = B * T

    def run(dev):
        from speech_diarization_amd import ops
        d = _conv_data(M * 131 + cout, M, cin, cout, k, B)
        d["x"][:, ::7] *= 1e-3                                              # small and large channels side by side
        x, w = d["x"].float(), d["w"].float()
        ws, s = ops.pack_weight_split16(w, dev)
        cp, f = ws.shape[2] * 32, float(2.0 ** s)
        if epilogues:
            ref = _ref_conv_cl(x.double(), w.double(), None, T, dil) + d["segb"].float().double().repeat_interleave(T, dim=0)
            ref = torch.tanh(torch.relu(ref) * d["scale"].float().double() + d["shift"].float().double())
        else:
            ref = torch.relu(_ref_conv_cl(x.double(), w.double(), d["b"].float().double(), T, dil)) * d["scale"].float().double() + d["shift"].float().double()

        def one(A):
            w_g = A.data(ws, "w_split")
            shift = A.data(d["shift"].float(), "shift")
            ldo, o_col0 = cout + 64, 32
            kw = {}
            if narrow:
                lda = cin + 12
                x_g, a_col0 = A.right(x, lda, "x")
                bias = A.data(d["segb"].float() if epilogues else d["b"].float(), "bias")
                scale = A.data(d["scale"].float(), "scale")
                kw.update(x_dtype=N.SD_DT_F32, w_scale_inv=1.0 / f)
            else:
                lda = cp + 64
                x_g, a_col0 = A.right(_split_rows(x, cp), 2 * lda, "x_split")
                a_col0 //= 2                                                # value columns
                bias, scale = A.data(d["b"].float() * f, "bias"), A.data(d["scale"].float() / f, "scale")
                kw.update(x_dtype=N.SD_DT_SPLIT16)
            res = {}
            if out_split:
                y, yv = A.out(M, 2 * cout, 2 * ldo, 2 * o_col0, F16, "y_split")
                kw.update(y=y, y_dtype=N.SD_DT_SPLIT16)
                res["y_split"] = yv
            else:
                y, yv = A.out(M, cout, ldo, o_col0, F32, "y")
                kw.update(y=y, y_dtype=N.SD_DT_F32)
                res["y"] = yv
            if epilogues:
                ta, ta_col0 = A.right(d["add"].float(), cout + 8, "tee_add")
                tee, tv = A.out(M, cout, cout + 24, 8, F32, "tee")
                kw.update(bias_per_seg=1, act2=_ACT["tanh"], tee=tee.ptr + 8 * 4, ldt=cout + 24, tee_lo=0, tee_hi=cout, tee_add=ta,
                          ld_ta=cout + 8, ta_col0=ta_col0)
                res["tee"] = tv
            a = _args(x=x_g, lda=lda, a_col0=a_col0, w=w_g, w_dtype=N.SD_DT_SPLIT16, ldo=ldo, o_col0=o_col0, M=M, T=T, cin=cin, cin_pad=cp,
                      cout=cout, taps=k, dil=dil, bias=bias, act=_ACT["relu"], scale=scale, shift=shift, **kw)
            ok("sd_conv1d_cl_split16", C.byref(a))
            return res
        got = under_poisons(dev, one)
        top = max(1.0, ref.abs().max().item())
        if out_split:           # bit for bit what sd_split16_pack_f32 makes of the f32 result (test_short_conv1d_cl_split16_matches_f64)
            halves = got["y_split"].view(M, cout // 32, 2, 32)
            val = halves[:, :, 0].float().double() + halves[:, :, 1].float().double()
            assert (val.reshape(M, cout) - ref).abs().max().item() < 2e-6 * top + 2.0 ** -21 * top
        else:
            assert (got["y"].double() - ref).abs().max().item() < 2e-6 * top
        if epilogues:           # test_short_conv1d_cl_split16_narrow_epilogues
            assert (got["tee"].double() - (ref + d["add"].float().double())).abs().max() < 4e-6
    return run


add("sd_conv1d_cl_split16", "narrow-0", _conv_split16(CONV_SHAPES[0], True))
add("sd_conv1d_cl_split16", "narrow-1", _conv_split16(CONV_SHAPES[1], True))
add("sd_conv1d_cl_split16", "narrow-3", _conv_split16(CONV_SHAPES[3], True))
add("sd_conv1d_cl_split16", "narrow-out-split", _conv_split16(CONV_SHAPES[3], True, out_split=True))
add("sd_conv1d_cl_split16", "narrow-epilogues", _conv_split16((9, 15, 128, 128, 3, 4), True, epilogues=True))
add("sd_conv1d_cl_split16", "wide-2", _conv_split16(CONV_SHAPES[2], False))
add("sd_conv1d_cl_split16", "wide-k1000", _conv_split16((3, 43, 1000, 1024, 3, 2), False))
add("sd_conv1d_cl_split16", "wide-out-split", _conv_split16((3, 43, 96, 1024, 1, 1), False, out_split=True))


def _split16_pack(M, c, ldx_extra, ldo_extra, mul):
    def run(dev):
        g = torch.Generator().manual_seed(M + c)
        x = torch.randn(M, c, generator=g) * torch.logspace(-4, 3, c)[None, :]
        cp = (c + 31) // 32 * 32
        ldo = cp + ldo_extra

        def one(A):
            x_g, col0 = A.right(x, c + ldx_extra, "x")
            o_g, ov = A.out_cut(M, 2 * cp, 2 * ldo, F16, "out")
            ok("sd_split16_pack_f32", x_g, c + ldx_extra, col0, M, c, mul, o_g, ldo)
            return {"out": ov}
        got = under_poisons(dev, one)["out"]
        want = _split_rows((x * mul).clamp(-65504, 65504), cp)
        assert torch.equal(got, want)                                       # hi = f16(v), lo = f16(v - hi): exact operations
    return run


add("sd_split16_pack_f32", "c80", _split16_pack(133, 80, 12, 32, 1.0))
add("sd_split16_pack_f32", "c1000-scaled", _split16_pack(129, 1000, 4, 0, 16.0))
add("sd_split16_pack_f32", "c36", _split16_pack(7, 36, 8, 64, 1.0))


def _conv_packed(T_list, cin, cout, k, dil, epilogues):
    M, B = sum(T_list), len(T_list)

    def run(dev):
        from speech_diarization_amd import ops
        d = _conv_data(M + k, M, cin, cout, k, B)
        x, w = d["x"].float(), d["w"].float()
        wp = ops.pack_weight(w, dev)
        fs = torch.from_numpy(np.concatenate([[0], np.cumsum(T_list)]).astype(np.int32))
        if epilogues:
            ref = _ref_conv_spans(x.double(), w.double(), None, T_list, dil) + d["segb"].float().double().repeat_interleave(torch.tensor(T_list), dim=0)
            ref = torch.sigmoid(torch.relu(ref))
        else:
            ref = torch.relu(_ref_conv_spans(x.double(), w.double(), d["b"].float().double(), T_list, dil)) * d["scale"].float().double() + d["shift"].float().double()

        def one(A):
            x_g, a_col0 = A.right(x, cin + 20, "x")
            w_g, fs_g = A.data(wp, "w"), A.data(fs, "frame_start")
            y, yv = A.out(M, cout, cout + 28, 12, F32, "y")
            res = {"y": yv}
            kw = dict(x=x_g, lda=cin + 20, a_col0=a_col0, w=w_g, y=y, ldo=cout + 28, o_col0=12, M=M, T=M, cin=cin, cin_pad=wp.shape[2], cout=cout,
                      taps=k, dil=dil, act=_ACT["relu"])
            if epilogues:
                ta, ta_col0 = A.right(d["add"].float(), cout + 8, "tee_add")
                tee, tv = A.out(M, cout, cout + 24, 8, F32, "tee")
                kw.update(bias=A.data(d["segb"].float(), "segb"), bias_per_seg=1, act2=_ACT["sigmoid"], tee=tee.ptr + 32, ldt=cout + 24, tee_lo=0,
                          tee_hi=cout, tee_add=ta, ld_ta=cout + 8, ta_col0=ta_col0)
                res["tee"] = tv
            else:
                kw.update(bias=A.data(d["b"].float(), "bias"), scale=A.data(d["scale"].float(), "scale"), shift=A.data(d["shift"].float(), "shift"))
            a = _args(**kw)
            ok("sd_conv1d_cl_packed_f32", C.byref(a), fs_g, B)
            return res
        got = under_poisons(dev, one)
        if epilogues:                                                       # test_packed_conv_epilogues_and_tile_counts
            assert (got["y"].double() - ref).abs().max() < 1e-5
            assert (got["tee"].double() - (ref + d["add"].float().double())).abs().max() < 1e-5
        else:                                                               # test_packed_conv_matches_f64
            assert (got["y"].double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    return run


add("sd_conv1d_cl_packed_f32", "stem-129-rows", _conv_packed([5, 7, 5, 9, 61, 42], 80, 192, 5, 1, False))
add("sd_conv1d_cl_packed_f32", "k1000-cout36", _conv_packed([5, 133, 9, 110], 1000, 36, 3, 4, False))
add("sd_conv1d_cl_packed_f32", "cout1100", _conv_packed([5, 7, 245], 80, 1100, 3, 2, False))
add("sd_conv1d_cl_packed_f32", "epilogues", _conv_packed([5, 7, 5, 9, 61, 42], 128, 128, 3, 4, True))
add("sd_conv1d_cl_packed_f32", "one-span", _conv_packed([5], 128, 128, 3, 4, True))


def _seg_gemm(M, cin, cout):
    def run(dev):
        from speech_diarization_amd import ops
        g = torch.Generator().manual_seed(M + cin)
        x = torch.randn(M, cin, generator=g, dtype=torch.float64)
        w = torch.randn(cout, cin, 1, generator=g, dtype=torch.float64) / np.sqrt(cin)
        b = torch.randn(cout, generator=g, dtype=torch.float64)
        scale = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5
        shift = torch.randn(cout, generator=g, dtype=torch.float64)
        ref = torch.sigmoid(torch.relu(x @ w[:, :, 0].T + b) * scale + shift)
        wp = ops.pack_weight(w.float(), dev)
        need = int(N.load().sd_seg_gemm_scratch_bytes(M, wp.shape[2], cout))
        assert (need > 0) == (M <= 256 and wp.shape[2] >= 512)

        def one(A):
            x_g, a_col0 = A.right(x.float(), cin + 8, "x")
            w_g, bias, sc, sh = A.data(wp, "w"), A.data(b.float(), "bias"), A.data(scale.float(), "scale"), A.data(shift.float(), "shift")
            y, yv = A.out(M, cout, cout + 12, 4, F32, "y")
            scr = A.scratch(need, "scratch")
            a = _args(x=x_g, lda=cin + 8, a_col0=a_col0, w=w_g, y=y, ldo=cout + 12, o_col0=4, M=M, T=1, cin=cin, cin_pad=wp.shape[2], cout=cout,
                      taps=1, dil=1, bias=bias, act=_ACT["relu"], scale=sc, shift=sh, act2=_ACT["sigmoid"])
            ok("sd_seg_gemm_f32", C.byref(a), scr.ptr if need else None, need)
            return {"y": yv}
        got = under_poisons(dev, one)["y"]
        assert (got.double() - ref).abs().max() < 2e-6                      # test_seg_gemm_matches_torch
    return run


for _M, _cin, _cout in [(32, 6144, 128), (16, 6144, 192), (128, 1024, 128), (7, 1000, 36), (200, 2080, 64), (300, 1024, 128), (5, 256, 64),
                        (225, 6144, 192), (256, 6144, 192)]:
    add("sd_seg_gemm_f32", f"M{_M}-K{_cin}-N{_cout}", _seg_gemm(_M, _cin, _cout))


def _chain_f64(r, layers, T):
    """float64 restatement with the path's own f16 roundings of the chain state (tests/test_gpu_short_segments.py)."""
    r = r.double().clone()
    n = len(layers)
    u = r[:, 128:256].clone()
    for j in range(1, n + 1):
        L = layers[j - 1]
        y = torch.relu(_ref_conv_cl(u, L["w"].double(), L["bias"].double(), T, L["dil"])) * L["scale"].double() + L["shift"].double()
        r[:, 128 * j:128 * j + 128] = y.half().double()
        if j < n:
            u = (y + r[:, 128 * (j + 1):128 * (j + 2)]).half().double()
    return r


def _res2net_chain(B, T, dil, n, ld):
    def run(dev):
        from speech_diarization_amd import ops
        lib = N.load()
        assert lib.sd_res2net_chain_supported(T, 128, n, 3, dil)
        g = torch.Generator().manual_seed(B * 1000 + T * 10 + dil)
        r = (torch.randn(B * T, ld, generator=g) * 0.7).half()
        layers = [dict(w=(torch.randn(128, 128, 3, generator=g) / np.sqrt(384)).half().float(), bias=torch.randn(128, generator=g) * 0.1,
                       scale=torch.rand(128, generator=g) + 0.5, shift=torch.randn(128, generator=g) * 0.1, dil=dil) for _ in range(n)]
        ref = _chain_f64(r, layers, T)
        need = int(lib.sd_res2net_chain_workspace_bytes(n))

        def one(A):
            r_g = A.data(r, "r")                                            # exactly [B*T][ld]: the chain runs in place on it
            arr = (N.sd_layer * n)()
            for L, d in zip(arr, layers):
                L.w, L.bias = A.data(ops.pack_weight(d["w"], dev, F16), "w").ptr, A.data(d["bias"], "bias").ptr
                L.scale, L.shift = A.data(d["scale"], "scale").ptr, A.data(d["shift"], "shift").ptr
                L.cin, L.cin_pad, L.cout, L.taps, L.dil, L.w_dtype = 128, 128, 128, 3, dil, N.SD_DT_F16
            ws = A.scratch(need, "ws")
            ok("sd_res2net_chain_f16", r_g, ld, B, T, arr, n, ws, need)
            return {"r": r_g.view(F16, B * T, ld)}
        got = under_poisons(dev, one)["r"].double()
        assert torch.equal(got[:, :128], r[:, :128].double()) and torch.equal(got[:, 128 * (n + 1):], r[:, 128 * (n + 1):].double())
        scale = ref[:, 128:128 * (n + 1)].abs().max().item()
        assert (got - ref)[:, 128:128 * (n + 1)].abs().max().item() < 4e-3 * scale       # test_short_res2net_chain_matches_f64_...
    return run


add("sd_res2net_chain_f16", "B7-T13-n7", _res2net_chain(7, 13, 3, 7, 1024))
add("sd_res2net_chain_f16", "B3-T212-n7", _res2net_chain(3, 212, 4, 7, 1024))
add("sd_res2net_chain_f16", "B5-T5-n3-ld520", _res2net_chain(5, 5, 4, 3, 520))


# ---- pooling / statistics / gating

def _pool_f64(logits, h, n_mask, eps=1e-12):
    B, T, Cc = h.shape
    mask = torch.arange(T)[None, :, None] < torch.as_tensor(n_mask)[:, None, None]
    a = torch.softmax(logits.masked_fill(~mask, float("-inf")), dim=1)
    mu = (a * h).sum(1)
    sd = torch.sqrt((a * (h - mu[:, None]) ** 2).sum(1).clamp_min(eps))
    return mu, sd


# (B, T, C): LDS-resident pooling, T too long for it (streaming), C not a multiple of 32 (streaming): the shapes of test_asp_pool
POOL_SHAPES = [(4, 201, 768), (2, 400, 256), (3, 50, 100)]


def _rel_for(B, T):
    rel = torch.tensor([1.0, 0.9 / T, 0.5, (T - 0.5) / T], dtype=F32)     # all, one frame, half, a length ending inside the last frame
    return rel[torch.arange(B) % 4].contiguous()


def _seg_rows(mode, B, T, T_list):
    """-> (M, rows of segment b as slices, frame_start tensor or None)"""
    if mode == "packed":
        fs = np.concatenate([[0], np.cumsum(T_list)]).astype(np.int64)
        return int(fs[-1]), [slice(int(fs[b]), int(fs[b + 1])) for b in range(len(T_list))], torch.from_numpy(fs.astype(np.int32))
    return B * T, [slice(b * T, (b + 1) * T) for b in range(B)], None


def _packed_T(B, T):
    """B spans around T frames, from the 5-frame floor."""
    g = np.random.default_rng(B * T)
    lst = g.integers(5, max(T, 7), B).tolist()
    lst[0], lst[-1] = 5, T
    return lst


def _mean_std(entry, mode, dt, B, T, Cc, want_std=True):
    def run(dev):
        from speech_diarization_amd.features import length_frames
        T_list = _packed_T(B, T)
        M, rows, fs = _seg_rows(mode, B, T, T_list)
        g = torch.Generator().manual_seed(11 + T)
        x = (torch.randn(M, Cc, generator=g) * 3 + 1).to(dt)
        rel = _rel_for(B, T)
        cnt = length_frames(rel, T)[1].tolist() if mode == "lens" else [r.stop - r.start for r in rows]
        ld = Cc + 12
        width = (2 if want_std else 1) * Cc

        def one(A):
            x_g, col0 = A.right(x, ld, "x")
            out = A.scratch(B * width * 4, "out")
            if entry == "sd_seg_mean_f32":
                ok(entry, x_g, ld, col0, B, T, Cc, out)
            elif entry == "sd_seg_mean_std_f32":
                ok(entry, x_g, ld, col0, B, T, Cc, 1e-12, out)
            elif mode == "uniform":
                ok(entry, x_g, _DT[dt], ld, col0, B, T, Cc, int(want_std), 1e-12, out)
            elif mode == "lens":
                ok(entry, x_g, _DT[dt], ld, col0, B, T, A.data(rel, "rel_len"), Cc, int(want_std), 1e-12, out)
            else:
                ok(entry, x_g, _DT[dt], ld, col0, A.data(fs, "frame_start"), B, M, Cc, int(want_std), 1e-12, out)
            return {"out": out.view(F32, B, width)}
        got = under_poisons(dev, one)["out"].double()
        for b in range(B):
            xs = x.double()[rows[b]][:cnt[b]]
            assert (got[b, :Cc] - xs.mean(0)).abs().max() < 1e-5            # test_segment_reductions_and_se / test_pool_kernels_on_f16_activations
            if want_std and cnt[b] > 1:
                assert (got[b, Cc:] - torch.sqrt(((xs - xs.mean(0)) ** 2).mean(0).clamp_min(1e-12))).abs().max() < 1e-5
    return run


def _se_scale(entry, mode, dt, B, T, Cc):
    def run(dev):
        T_list = _packed_T(B, T)
        M, rows, fs = _seg_rows(mode, B, T, T_list)
        g = torch.Generator().manual_seed(5 + T)
        x = (torch.randn(M, Cc, generator=g) * 2 + 0.5).to(dt)
        res = torch.randn(M, Cc, generator=g).to(dt)
        gate = torch.rand(B, Cc, generator=g)
        v = 8 if dt == F16 else 4
        ldx, ldr, ldy, y_col0 = Cc + 2 * v, Cc + 3 * v, Cc + 5 * v, 2 * v
        ref = torch.cat([x.double()[rows[b]] * gate[b].double() + res.double()[rows[b]] for b in range(B)])

        def one(A):
            x_g = A.cut(x, ldx, "x")
            r_g, r_col0 = A.right(res, ldr, "res")
            gate_g = A.data(gate, "gate")
            y, yv = A.out(M, Cc, ldy, y_col0, dt, "y")
            if entry == "sd_se_scale_residual_f32":
                ok(entry, x_g, ldx, gate_g, r_g, ldr, r_col0, y, ldy, y_col0, B, T, Cc)
            elif mode == "uniform":
                ok(entry, x_g, ldx, gate_g, r_g, ldr, r_col0, y, ldy, y_col0, B, T, Cc, _DT[dt])
            else:
                ok(entry, x_g, ldx, gate_g, r_g, ldr, r_col0, y, ldy, y_col0, A.data(fs, "frame_start"), B, M, Cc, _DT[dt])
            return {"y": yv}
        got = under_poisons(dev, one)["y"].double()
        assert (got - ref).abs().max() < (1e-2 if dt == F16 else 1e-5)      # test_pool_kernels_on_f16_activations / test_segment_reductions_and_se
    return run


def _asp_pool(entry, mode, dt, B, T, Cc):
    def run(dev):
        from speech_diarization_amd.features import length_frames
        T_list = _packed_T(B, T)
        M, rows, fs = _seg_rows(mode, B, T, T_list)
        g = torch.Generator().manual_seed(3 + T)
        logit = (torch.randn(M, Cc, generator=g) * 4).to(dt)
        h = torch.randn(M, Cc, generator=g).to(dt)
        rel = _rel_for(B, T)
        cnt = length_frames(rel, T)[1].tolist() if mode == "lens" else [r.stop - r.start for r in rows]
        ldl, ldh = Cc + 8, Cc + 16

        def one(A):
            l_g, h_g = A.cut(logit, ldl, "logit"), A.cut(h, ldh, "h")
            out = A.scratch(B * 2 * Cc * 4, "out")
            if entry == "sd_asp_pool_f32":
                ok(entry, l_g, ldl, h_g, ldh, B, T, Cc, 1e-12, out)
            elif mode == "uniform":
                ok(entry, l_g, ldl, h_g, _DT[dt], ldh, B, T, Cc, 1e-12, out)
            elif mode == "lens":
                ok(entry, l_g, ldl, h_g, _DT[dt], ldh, B, T, A.data(rel, "rel_len"), Cc, 1e-12, out)
            else:
                ok(entry, l_g, ldl, h_g, _DT[dt], ldh, A.data(fs, "frame_start"), B, M, Cc, 1e-12, out)
            return {"out": out.view(F32, B, 2 * Cc)}
        got = under_poisons(dev, one)["out"].double()
        for b in range(B):
            n = rows[b].stop - rows[b].start
            mu, sd = _pool_f64(logit.double()[rows[b]].view(1, n, Cc), h.double()[rows[b]].view(1, n, Cc), [cnt[b]])
            bar = 1e-5 if dt == F32 else 2e-5                               # test_asp_pool / test_short_asp_pool_and_seg_mean_std_match_f64
            assert (got[b, :Cc] - mu[0]).abs().max() < bar
            if cnt[b] > 1:
                assert (got[b, Cc:] - sd[0]).abs().max() < bar
    return run


for _B, _T, _C in POOL_SHAPES:
    _id = f"B{_B}-T{_T}-C{_C}"
    add("sd_seg_mean_f32", _id, _mean_std("sd_seg_mean_f32", "uniform", F32, _B, _T, _C, want_std=False))
    add("sd_seg_mean_std_f32", _id, _mean_std("sd_seg_mean_std_f32", "uniform", F32, _B, _T, _C))
    add("sd_se_scale_residual_f32", _id, _se_scale("sd_se_scale_residual_f32", "uniform", F32, _B, _T, _C if _C % 8 == 0 else 104))
    add("sd_asp_pool_f32", _id, _asp_pool("sd_asp_pool_f32", "uniform", F32, _B, _T, _C))
    for _dt, _n in ((F32, "f32"), (F16, "f16")):
        add("sd_seg_mean_std_dt", f"{_n}-{_id}", _mean_std("sd_seg_mean_std_dt", "uniform", _dt, _B, _T, _C))
        add("sd_seg_mean_std_lens_dt", f"{_n}-{_id}", _mean_std("sd_seg_mean_std_lens_dt", "lens", _dt, _B, _T, _C))
        add("sd_seg_mean_std_packed_dt", f"{_n}-{_id}", _mean_std("sd_seg_mean_std_packed_dt", "packed", _dt, _B, _T, _C))
        add("sd_se_scale_residual_dt", f"{_n}-{_id}", _se_scale("sd_se_scale_residual_dt", "uniform", _dt, _B, _T, _C if _C % 8 == 0 else 104))
        add("sd_se_scale_residual_packed_dt", f"{_n}-{_id}", _se_scale("sd_se_scale_residual_packed_dt", "packed", _dt, _B, _T, _C if _C % 8 == 0 else 104))
        add("sd_asp_pool_dt", f"{_n}-{_id}", _asp_pool("sd_asp_pool_dt", "uniform", _dt, _B, _T, _C))
        add("sd_asp_pool_lens_dt", f"{_n}-{_id}", _asp_pool("sd_asp_pool_lens_dt", "lens", _dt, _B, _T, _C))
        add("sd_asp_pool_packed_dt", f"{_n}-{_id}", _asp_pool("sd_asp_pool_packed_dt", "packed", _dt, _B, _T, _C))
add("sd_seg_mean_std_dt", "f32-mean-only", _mean_std("sd_seg_mean_std_dt", "uniform", F32, 5, 37, 256, want_std=False))


def _attend_pool(mode, lens, B, T, Cc):
    """a1 [B*T][att] contiguous (exactly), wc exactly [C][1][att], h with a row stride."""
    def run(dev):
        from speech_diarization_amd import ops
        from speech_diarization_amd.features import length_frames
        att = 128
        g = torch.Generator().manual_seed(T * 10 + lens)
        dtype = F16 if mode == "f16" else F32
        a1 = torch.tanh(torch.randn(B * T, att, generator=g)).to(dtype)
        wc = (torch.randn(Cc, att, 1, generator=g) / 4).to(dtype)
        h = (torch.randn(B * T, Cc, generator=g) * 1.5 + 0.3).to(dtype)
        rel = _rel_for(B, T)
        n_mask = length_frames(rel, T)[1] if lens else torch.full((B,), T)
        wp = ops.pack_weight(wc.float(), dev, dtype)
        dt = {"f32": N.SD_DT_F32, "f16": N.SD_DT_F16, "split16": N.SD_DT_SPLIT16}[mode]
        assert N.load().sd_asp_attend_pool_supported(N.SD_DT_F16 if mode == "f16" else N.SD_DT_F32, T, Cc, att)
        ldh = Cc + 16

        def one(A):
            a_g, w_g, h_g = A.data(a1, "a1"), A.data(wp, "wc"), A.cut(h, ldh, "h")
            out = A.scratch(B * 2 * Cc * 4, "out")
            if lens:
                ok("sd_asp_attend_pool_lens_dt", a_g, w_g, h_g, dt, ldh, B, T, A.data(rel, "rel_len"), Cc, att, 1e-12, out)
            else:
                ok("sd_asp_attend_pool_dt", a_g, w_g, h_g, dt, ldh, B, T, Cc, att, 1e-12, out)
            return {"out": out.view(F32, B, 2 * Cc)}
        got = under_poisons(dev, one)["out"].double()
        logits = (a1.double() @ wc[:, :, 0].double().T).view(B, T, Cc)
        mu, sd = _pool_f64(logits, h.double().view(B, T, Cc), n_mask)
        assert (got[:, :Cc] - mu).abs().max() < 2e-5                        # test_short_fused_attention_pooling_matches_f64
        if mode == "f16":
            mask = torch.arange(T)[None, :, None] < n_mask[:, None, None]
            e2 = (torch.softmax(logits.masked_fill(~mask, float("-inf")), dim=1) * h.double().view(B, T, Cc) ** 2).sum(1)
            sd_bar = e2 * 2.0 ** -21 / (2 * sd) + 2e-4
        else:
            sd_bar = torch.full_like(sd, 2e-5)
        live = n_mask > 1
        assert bool(((got[live, Cc:] - sd[live]).abs() < sd_bar[live]).all())
    return run


def _asp_T_limits():
    """(last T the fused pooling accepts, first it refuses), asked of the library."""
    lib = N.load()
    T = 1
    while lib.sd_asp_attend_pool_supported(N.SD_DT_F32, T + 1, 512, 128) and T < 100000:
        T += 1
    return T, T + 1


def _chain_T_limits():
    lib = N.load()
    T = 5
    while lib.sd_res2net_chain_supported(T + 1, 128, 7, 3, 4) and T < 100000:
        T += 1
    return T, T + 1


for _mode in ("f32", "f16", "split16"):
    add("sd_asp_attend_pool_dt", f"{_mode}-T7", _attend_pool(_mode, False, 5, 7, 512))
    add("sd_asp_attend_pool_dt", f"{_mode}-T201", _attend_pool(_mode, False, 3, 201, 768))
    add("sd_asp_attend_pool_lens_dt", f"{_mode}-T7", _attend_pool(_mode, True, 5, 7, 512))
    add("sd_asp_attend_pool_lens_dt", f"{_mode}-T201", _attend_pool(_mode, True, 4, 201, 256))


@case("sd_asp_attend_pool_dt", "last-supported-T")
def _attend_pool_at_its_limit(dev):
    _attend_pool("f32", False, 2, _asp_T_limits()[0], 256)(dev)
    _attend_pool("f16", False, 2, _asp_T_limits()[0], 256)(dev)


@case("sd_wav_lens_frames", "counts")
def _wav_lens_frames(dev):
    from speech_diarization_amd.features import length_frames
    T = 201
    rel = torch.tensor([1.0, 0.9 / T, 0.5, (T - 0.5) / T, 100.3 / T, 0.0, 1e-9], dtype=F32)
    B = rel.numel()

    def one(A):
        r_g = A.data(rel, "rel_len")
        nn_, nm = A.scratch(B * 4, "n_norm"), A.scratch(B * 4, "n_mask")
        ok("sd_wav_lens_frames", r_g, B, T, nn_, nm)
        only = A.scratch(B * 4, "n_mask alone")
        ok("sd_wav_lens_frames", r_g, B, T, None, only)
        return {"n_norm": nn_.view(I32), "n_mask": nm.view(I32), "only": only.view(I32)}
    got = under_poisons(dev, one)
    n_norm, n_mask = length_frames(rel, T)
    assert got["n_norm"].tolist() == n_norm.tolist() and got["n_mask"].tolist() == n_mask.tolist() == got["only"].tolist()


# ---- cosine / affinity / scores

def _cosine(entry, n, d, rows=None, pad=4):
    def run(dev):
        from sklearn.metrics.pairwise import cosine_similarity
        lib = N.load()
        rng = np.random.default_rng(n + d)
        x = rng.standard_normal((n, d)).astype(np.float32) * rng.uniform(0.01, 30.0, size=(n, 1)).astype(np.float32)
        if n > 7:
            x[7] = 0.0
        ref = cosine_similarity(x.astype(np.float64))
        split = entry.endswith("split16")
        need = int((lib.sd_cosine_split16_workspace_bytes if split else lib.sd_cosine_workspace_bytes)(n, d))
        lo, hi = rows if rows is not None else (0, n)

        def one(A):
            x_g = A.data(torch.from_numpy(x), "x")
            ws = A.scratch(need, "ws")
            o_g, ov = A.out_cut(hi - lo, n, n + pad, F32, "out")
            if entry == "sd_cosine_affinity_f32":
                ok(entry, x_g, n, d, o_g, n + pad, ws, need)
            else:
                ok(entry, x_g, n, d, lo, hi, o_g, n + pad, ws, need)
            return {"out": ov}
        got = under_poisons(dev, one)["out"].numpy()
        assert np.abs(got - ref[lo:hi]).max() < 2e-6                        # test_cosine_affinity_matches_sklearn / _split16_
        if n > 7 and lo <= 7 < hi:
            assert np.all(got[7 - lo] == 0.0)
    return run


for _n in (1, 129, 1500, 3001):
    for _d in (7, 50, 192):
        add("sd_cosine_affinity_f32", f"n{_n}-d{_d}", _cosine("sd_cosine_affinity_f32", _n, _d, pad=0 if _n == 1500 else 4))
        _lo = max(0, _n - 131)
        add("sd_cosine_affinity_rows_f32", f"n{_n}-d{_d}-last-rows", _cosine("sd_cosine_affinity_rows_f32", _n, _d, rows=(_lo, _n)))
        add("sd_cosine_affinity_rows_split16", f"n{_n}-d{_d}-last-rows", _cosine("sd_cosine_affinity_rows_split16", _n, _d, rows=(_lo, _n)))
add("sd_cosine_affinity_f32", "n3001-unaligned-rows", _cosine("sd_cosine_affinity_f32", 3001, 192, pad=3))
add("sd_cosine_affinity_rows_split16", "n1500-whole", _cosine("sd_cosine_affinity_rows_split16", 1500, 192, rows=(0, 1500), pad=0))
add("sd_cosine_affinity_rows_split16", "n3001-whole", _cosine("sd_cosine_affinity_rows_split16", 3001, 192, rows=(0, 3001), pad=3))
add("sd_cosine_affinity_rows_f32", "n1500-middle", _cosine("sd_cosine_affinity_rows_f32", 1500, 192, rows=(686, 950)))


def _l2norm(n, d, ldx, ldo):
    def run(dev):
        rng = np.random.default_rng(n * d)
        x = rng.standard_normal((n, d)).astype(np.float32)
        if n > 3:
            x[3] = 0.0

        def one(A):
            x_g = A.cut(torch.from_numpy(x), ldx, "x")
            o_g = A.scratch(n * ldo * 4, "xn")                              # columns [D, ldo) are zero filled: the whole [N][ldo] is written
            ok("sd_l2norm_rows_f32", x_g, ldx, n, d, 1e-8, 0, o_g, ldo)
            s_g = A.scratch(n * ldo * 4, "xn sklearn")
            ok("sd_l2norm_rows_f32", x_g, ldx, n, d, 0.0, 1, s_g, ldo)
            return {"xn": o_g.view(F32, n, ldo), "sk": s_g.view(F32, n, ldo)}
        got = under_poisons(dev, one)
        x64 = x.astype(np.float64)
        nrm = np.linalg.norm(x64, axis=1, keepdims=True)
        assert np.abs(got["xn"].numpy()[:, :d] - x64 / (nrm + 1e-8)).max() < 1e-6
        assert np.abs(got["sk"].numpy()[:, :d] - x64 / np.where(nrm == 0, 1.0, nrm)).max() < 1e-6
        assert bool((got["xn"][:, d:] == 0).all()) and bool((got["sk"][:, d:] == 0).all())
    return run


add("sd_l2norm_rows_f32", "n41-d192", _l2norm(41, 192, 200, 192))
add("sd_l2norm_rows_f32", "n129-d50-padded", _l2norm(129, 50, 53, 64))
add("sd_l2norm_rows_f32", "n1-d7", _l2norm(1, 7, 7, 32))


def _adjacent_and_argmax(n, d, K, ld_extra):
    def run(dev):
        from oracle.pipeline_ref import adjacent_cosine_ref, assign_windows_ref
        rng = np.random.default_rng(n + K)
        e = rng.standard_normal((n, d)).astype(np.float32)
        c = rng.standard_normal((K, d)).astype(np.float32)
        c /= np.linalg.norm(c, axis=1, keepdims=True)
        wn = (e.astype(np.float64) / (np.linalg.norm(e.astype(np.float64), axis=1, keepdims=True) + 1e-8)).astype(np.float32)

        def one(A):
            e_g = A.cut(torch.from_numpy(e), d + ld_extra, "x")
            sims = A.scratch(max(n - 1, 0) * 4, "sims")
            ok("sd_adjacent_cosine_f32", e_g, d + ld_extra, n, d, 1e-8, sims)
            w_g, c_g = A.cut(torch.from_numpy(wn), d + ld_extra, "w"), A.cut(torch.from_numpy(c), d + 2 * ld_extra, "c")
            best, score = A.scratch(n * 4, "best"), A.scratch(n * 4, "score")
            ok("sd_sim_argmax_f32", w_g, d + ld_extra, n, d, c_g, d + 2 * ld_extra, K, best, score)
            return {"sims": sims.view(F32), "best": best.view(I32), "score": score.view(F32)}
        got = under_poisons(dev, one)
        if n > 1:
            assert np.abs(got["sims"].numpy() - adjacent_cosine_ref(e.astype(np.float64))).max() < 1e-6     # test_adjacent_cosine_and_argmax
        ref_best, ref_sim = assign_windows_ref(e.astype(np.float64), c.astype(np.float64))
        assert np.array_equal(got["best"].numpy(), ref_best)
        assert np.abs(got["score"].numpy() - ref_sim.max(1)).max() < 1e-6
    return run


for _e in ("sd_adjacent_cosine_f32", "sd_sim_argmax_f32"):
    add(_e, "n41-d192-k5", _adjacent_and_argmax(41, 192, 5, 0))
    add(_e, "n129-d50-k3-strided", _adjacent_and_argmax(129, 50, 3, 3))
    add(_e, "n2-d7-k1", _adjacent_and_argmax(2, 7, 1, 1))


def _topk(rows, n, k, ld):
    def run(dev):
        rng = np.random.default_rng(3 + n)
        x = rng.standard_normal((rows, n)).astype(np.float32)
        x[0, : n // 3] = x[0, 0]
        if rows > 1:
            x[1] = 0.25

        def one(A):
            x_g = A.cut(torch.from_numpy(x), ld, "x")                        # row stride > n: the gap is 0xFF (a NaN that would enter the top-k)
            out = A.scratch(rows * 2 * 4, "out")
            ok("sd_topk_mean_std_f32", x_g, ld, rows, n, k, out)
            return {"out": out.view(F32, rows, 2)}
        got = under_poisons(dev, one)["out"].numpy()
        top = np.sort(x.astype(np.float64), axis=1)[:, -min(k, n):]
        assert np.allclose(got[:, 0], top.mean(1), atol=2e-6) and np.allclose(got[:, 1], top.std(1), atol=2e-6)   # test_topk_mean_std_matches_numpy
    return run


for _rows, _n, _k, _ld in [(7, 64, 20, 64), (3, 1000, 200, 1003), (5, 10000, 200, 10240), (2, 50, 200, 51), (4, 257, 1, 512), (1, 300, 300, 300)]:
    add("sd_topk_mean_std_f32", f"rows{_rows}-n{_n}-k{_k}", _topk(_rows, _n, _k, _ld))


def _asnorm(nq, nr, ld, ldo):
    def run(dev):
        rng = np.random.default_rng(nq + nr)
        raw = rng.standard_normal((nq, nr)).astype(np.float32)
        qs = np.stack([rng.standard_normal(nq), rng.uniform(0.1, 2.0, nq)], axis=1).astype(np.float32)
        rs = np.stack([rng.standard_normal(nr), rng.uniform(0.1, 2.0, nr)], axis=1).astype(np.float32)

        def one(A):
            raw_g = A.cut(torch.from_numpy(raw), ld, "raw")
            q_g, r_g = A.data(torch.from_numpy(qs), "qstat"), A.data(torch.from_numpy(rs), "rstat")
            o_g, ov = A.out_cut(nq, nr, ldo, F32, "out")
            ok("sd_asnorm_combine_f32", raw_g, ld, nq, nr, q_g, r_g, o_g, ldo)
            return {"out": ov}
        got = under_poisons(dev, one)["out"].numpy()
        r64, q64, s64 = raw.astype(np.float64), qs.astype(np.float64), rs.astype(np.float64)
        ref = 0.5 * ((r64 - q64[:, :1]) / (q64[:, 1:] + 1e-6) + (r64 - s64[:, 0][None]) / (s64[:, 1][None] + 1e-6))
        assert np.abs(got - ref).max() < 2e-4 * max(1.0, np.abs(ref).max())   # the bar of test_asnorm_scores_gpu_matches_reference_goldens_and_host
    return run


add("sd_asnorm_combine_f32", "nq500-nr6", _asnorm(500, 6, 6, 7))
add("sd_asnorm_combine_f32", "nq37-nr129", _asnorm(37, 129, 131, 129))


def _viterbi(T, K, alpha, ld):
    def run(dev):
        from speech_diarization_amd import diar_diag as dd
        rng = np.random.default_rng(4 + T)
        sc = rng.standard_normal((T, K)).astype(np.float32)
        sc[::7] = np.round(sc[::7])
        need = int(N.load().sd_viterbi_workspace_bytes(T, K))
        log_move = float(np.float32(np.log((1 - alpha) / (K - 1) + 1e-8))) if K > 1 else 0.0
        log_stay = float(np.float32(np.log(alpha + 1e-8)))

        def one(A):
            s_g = A.cut(torch.from_numpy(sc), ld, "scores")
            ws, path = A.scratch(need, "ws"), A.scratch(T * 4, "path")
            ok("sd_viterbi_f32", s_g, ld, T, K, log_stay, log_move, ws, need, path)
            return {"path": path.view(I32)}
        got = under_poisons(dev, one)["path"]
        assert got.tolist() == dd.viterbi_hmm(sc, alpha).tolist()           # test_viterbi_gpu_path_equals_the_reference_path
    return run


for _T, _K, _a, _ld in [(1, 3, 0.9, 3), (2, 2, 0.995, 5), (129, 8, 0.9, 8), (1000, 16, 0.995, 17), (36000, 8, 0.995, 8), (300, 1, 0.9, 2), (257, 64, 0.9, 64)]:
    add("sd_viterbi_f32", f"T{_T}-K{_K}", _viterbi(_T, _K, _a, _ld))


def test_misaligned_slices_are_refused_before_launch(dev):
    """Offsets that miss an entry's documented INPUT alignment (multiples of 4 values for f32, 8 for f16, 32 for SD_DT_SPLIT16 rows): SD_ERR_ARG,
    nothing launched -- every output keeps its poison, guards intact.  (An OUTPUT slice that misses the 16-byte alignment takes the scalar
    epilogue instead: the "unaligned-out" cases of the table.)"""
    from speech_diarization_amd import ops
    lib = N.load()
    A = Arena(dev, 0x7B)
    M, T, cin, cout = 26, 13, 64, 64
    x32, x16 = A.scratch(M * (cin + 64) * 4, "x f32"), A.scratch(M * (cin + 64) * 2, "x f16")
    w32 = A.data(ops.pack_weight(torch.zeros(cout, cin, 1), dev), "w")
    w16 = A.data(ops.pack_weight(torch.zeros(cout, cin, 1), dev, F16), "w f16")
    ws16 = A.data(ops.pack_weight_split16(torch.ones(cout, cin, 1), dev)[0], "w split")
    outs = []

    def out(nbytes, name):
        outs.append(A.scratch(nbytes, name))
        return outs[-1]

    def conv(entry, **kw):
        a = _args(M=M, T=T, cin=cin, cout=cout, taps=1, dil=1, ldo=cout, **kw)
        return call(entry, C.byref(a))
    assert conv("sd_conv1d_cl_f32", x=x32, lda=cin + 8, a_col0=2, w=w32, cin_pad=64, y=out(M * cout * 4, "y")) == -1 and "multiples of 4" in N.last_error()
    assert conv("sd_conv1d_cl_f32", x=x32, lda=cin + 6, a_col0=4, w=w32, cin_pad=64, y=out(M * cout * 4, "y")) == -1
    assert conv("sd_conv1d_cl_f16", x=x16, lda=cin + 16, a_col0=4, x_dtype=N.SD_DT_F16, w=w16, w_dtype=N.SD_DT_F16, cin_pad=64,
                y=out(M * cout * 2, "y"), y_dtype=N.SD_DT_F16) == -1 and "multiples of 8" in N.last_error()
    assert conv("sd_conv1d_cl_split16", x=x32, lda=cin + 32, a_col0=16, x_dtype=N.SD_DT_SPLIT16, w=ws16, w_dtype=N.SD_DT_SPLIT16, cin_pad=64,
                y=out(M * cout * 4, "y")) == -1 and "multiples of 32" in N.last_error()
    assert conv("sd_conv1d_cl_split16", x=x32, lda=cin + 8, a_col0=2, x_dtype=N.SD_DT_F32, w=ws16, w_dtype=N.SD_DT_SPLIT16, cin_pad=64,
                y=out(M * cout * 4, "y")) == -1
    fs = A.data(torch.tensor([0, 13, 26], dtype=I32), "frame_start")
    a = _args(M=M, T=M, cin=cin, cout=cout, taps=1, dil=1, ldo=cout, x=x32, lda=cin + 8, a_col0=2, w=w32, cin_pad=64, y=out(M * cout * 4, "y"))
    assert lib.sd_conv1d_cl_packed_f32(C.byref(a), fs.ptr, 2, _stream()) == -1
    assert call("sd_split16_pack_f32", x32, cin + 8, 2, M, cin, 1.0, out(M * 2 * cin * 2, "packed"), cin) == -1
    for dt, xb in ((N.SD_DT_F32, x32), (N.SD_DT_F16, x16)):
        assert call("sd_seg_mean_std_dt", xb, dt, cin + 8, 2, 2, T, cin, 1, 1e-12, out(2 * 2 * cin * 4, "stats")) == -1
        assert call("sd_seg_mean_std_packed_dt", xb, dt, cin + 8, 2, fs, 2, M, cin, 1, 1e-12, out(2 * 2 * cin * 4, "stats")) == -1
    gate = A.scratch(2 * cin * 4, "gate")
    assert call("sd_se_scale_residual_dt", x16, cin + 16, gate, x16, cin + 16, 0, out(M * (cin + 16) * 2, "y"), cin + 16, 4, 2, T, cin, N.SD_DT_F16) == -1
    assert call("sd_se_scale_residual_dt", x32, cin + 16, gate, x32, cin + 16, 2, out(M * (cin + 16) * 4, "y"), cin + 16, 0, 2, T, cin, N.SD_DT_F32) == -1
    r = out(10 * 1028 * 2, "r")
    layers = (N.sd_layer * 7)()
    cw = A.scratch(int(lib.sd_res2net_chain_workspace_bytes(7)), "chain ws")
    assert lib.sd_res2net_chain_f16(r.ptr, 1028, 2, 5, layers, 7, cw.ptr, cw.nbytes, _stream()) == -1
    torch.cuda.synchronize()
    for o in outs + [cw]:
        assert bool((o.payload == 0x7B).all()), o.name
    A.check()


# ====================================================================== 2. fbank, every route

_PLANS = {}


def _plan(kind, sr=16000):
    from speech_diarization_amd.features import FbankPlan
    if (kind, sr) not in _PLANS:
        _PLANS[(kind, sr)] = FbankPlan(kind, sr=sr) if sr != 16000 else FbankPlan(kind)
    return _PLANS[(kind, sr)]


def _wav(seed, B, n):
    from speech_diarization_amd import synth
    wav = synth.synthetic_segments(seed, B, n, std=0.2)
    if B > 1:
        wav[1, n // 3: 2 * n // 3] *= 1e-3
    return torch.from_numpy(wav)


def _fbank(kind, sr, B, n, mean_norm=True):
    """wav exactly [B][n] (the last row's last frame ends at the guard), workspace exactly sd_fbank_workspace_bytes, out with a row stride
    of n_mels + 8; bitwise `fbank_device` on plain tensors."""
    def run(dev):
        from speech_diarization_amd.engine import fbank_device
        plan = _plan(kind, sr)
        wav = _wav(n + B, B, n)
        T, nm = plan.frames(n), plan.n_mels
        need = int(N.load().sd_fbank_workspace_bytes(plan.handle, B, n))
        want = fbank_device(wav.to(dev), plan, mean_norm=mean_norm).cpu()

        def one(A):
            w_g, ws = A.data(wav, "wav"), A.scratch(need, "ws")
            o_g, ov = A.out_cut(B * T, nm, nm + 8, F32, "out")
            ok("sd_fbank_f32", plan.handle, w_g, B, n, int(mean_norm), o_g, nm + 8, ws, need)
            return {"out": ov}
        got = under_poisons(dev, one)["out"]
        assert torch.equal(got.view(B, T, nm), want)
    return run


for _kind in ("speechbrain", "torchaudio"):
    for _n in (801, 3203, 16001, 32000, 32100, 32102, 32160, 35003):       # both sides of the one-launch / folded switch (201 frames)
        add("sd_fbank_f32", f"{_kind}-n{_n}", _fbank(_kind, 16000, 3, _n))
    add("sd_fbank_f32", f"{_kind}-raw-n32000", _fbank(_kind, 16000, 2, 32000, mean_norm=False))
    add("sd_fbank_f32", f"{_kind}-one-row-n640", _fbank(_kind, 16000, 1, 640))
for _sr, _n in ((8000, 4000), (22050, 11025), (48000, 9600)):
    add("sd_fbank_f32", f"generic-sr{_sr}", _fbank("torchaudio", _sr, 3, _n))
add("sd_fbank_f32", "generic-more-than-one-workspace-chunk", _fbank("torchaudio", 48000, 150, 48000))


def _fbank_windows(kind, sr, n_total, n, starts):
    def run(dev):
        from speech_diarization_amd.engine import fbank_device
        plan = _plan(kind, sr)
        sig = _wav(n_total, 1, n_total)[0]
        B = len(starts)
        T, nm = plan.frames(n), plan.n_mels
        need = int(N.load().sd_fbank_workspace_bytes(plan.handle, B, n))
        rows = torch.zeros(B, n)
        for i, s in enumerate(starts):
            lo, hi = max(s, 0), min(s + n, n_total)
            rows[i, lo - s:hi - s] = sig[lo:hi]
        want = fbank_device(rows.to(dev), plan).cpu()

        def one(A):
            s_g, st_g, ws = A.data(sig, "signal"), A.data(torch.tensor(starts, dtype=I64), "starts"), A.scratch(need, "ws")
            o_g, ov = A.out_cut(B * T, nm, nm + 8, F32, "out")
            ok("sd_fbank_windows_f32", plan.handle, s_g, n_total, st_g, B, n, 1, o_g, nm + 8, ws, need)
            return {"out": ov}
        assert torch.equal(under_poisons(dev, one)["out"].view(B, T, nm), want)
    return run


# windows hanging over both ends of the signal, one ending on its last sample
add("sd_fbank_windows_f32", "speechbrain-one-launch", _fbank_windows("speechbrain", 16000, 40000, 16000, [0, 777, 24000, 39000, -300, -15999, 39999]))
add("sd_fbank_windows_f32", "torchaudio-one-launch", _fbank_windows("torchaudio", 16000, 40000, 16000, [0, 777, 24000, 39000, -300]))
add("sd_fbank_windows_f32", "speechbrain-folded", _fbank_windows("speechbrain", 16000, 70000, 35003, [0, 34997, 60000, -20000]))
add("sd_fbank_windows_f32", "generic-8k", _fbank_windows("torchaudio", 8000, 40000, 4000, [0, 777, 36000, 39000, -300]))


def _fbank_lens(B, n):
    def run(dev):
        plan = _plan("speechbrain")
        wav = _wav(n, B, n)
        T, nm = plan.frames(n), plan.n_mels
        rel = _rel_for(B, T)
        need = int(N.load().sd_fbank_workspace_bytes(plan.handle, B, n))
        wd, rd = wav.to(dev), rel.to(dev)
        plain, pws = torch.empty(B, T, nm, device=dev), torch.empty(max(need, 256), dtype=U8, device=dev)
        ok("sd_fbank_lens_f32", plan.handle, wd, B, n, rd, plain, nm, pws, pws.numel())
        torch.cuda.synchronize()

        def one(A):
            w_g, r_g, ws = A.data(wav, "wav"), A.data(rel, "rel_len"), A.scratch(need, "ws")
            o_g, ov = A.out_cut(B * T, nm, nm + 8, F32, "out")
            ok("sd_fbank_lens_f32", plan.handle, w_g, B, n, r_g, o_g, nm + 8, ws, need)
            return {"out": ov}
        got = under_poisons(dev, one)["out"].view(B, T, nm)
        assert torch.equal(got, plain.cpu())
        # the masked mean against float64: raw features (this library, mean_norm = 0) minus the mean over the first n_norm frames
        from speech_diarization_amd.engine import fbank_device
        from speech_diarization_amd.features import length_frames
        raw = fbank_device(wd, plan, mean_norm=False).cpu().double()
        n_norm = length_frames(rel, T)[0].tolist()
        ref = torch.stack([raw[b] - raw[b, :n_norm[b]].mean(0) for b in range(B)])
        assert (got.double() - ref).abs().max() < 1e-4
    return run


add("sd_fbank_lens_f32", "one-launch-n32000", _fbank_lens(5, 32000))
add("sd_fbank_lens_f32", "folded-n35003", _fbank_lens(4, 35003))
add("sd_fbank_lens_f32", "floor-n640", _fbank_lens(3, 640))


def _fbank_packed(n_total, spans):
    def run(dev):
        from speech_diarization_amd.engine import fbank_device, span_frame_offsets
        plan = _plan("speechbrain")
        sig = _wav(n_total + 1, 1, n_total)[0]
        starts, lens = [s for s, _ in spans], [n for _, n in spans]
        fs = span_frame_offsets(lens)
        B, M, n_max, nm = len(spans), int(fs[-1]), max(lens), plan.n_mels
        need = int(N.load().sd_fbank_packed_workspace_bytes(plan.handle, B, M, n_max))
        sd_ = sig.to(dev)

        def one(A):
            s_g, ws = A.data(sig, "signal"), A.scratch(need, "ws")
            st_g, ln_g = A.data(torch.tensor(starts, dtype=I64), "starts"), A.data(torch.tensor(lens, dtype=I32), "lens")
            fs_g = A.data(torch.from_numpy(fs), "frame_start")
            o_g, ov = A.out_cut(M, nm, nm + 8, F32, "out")
            ok("sd_fbank_packed_f32", plan.handle, s_g, n_total, st_g, ln_g, fs_g, B, M, n_max, o_g, nm + 8, ws, need)
            return {"out": ov}
        got = under_poisons(dev, one)["out"]
        for s, (a, n) in enumerate(spans):                                  # bitwise the span alone (test_fbank_packed_is_bitwise_the_span_alone)
            alone = fbank_device(sd_[a:a + n].contiguous()[None], plan)[0].cpu()
            assert torch.equal(got[fs[s]:fs[s + 1]], alone), (s, a, n)
    return run


# overlapping spans, both routes in one pack, a span that ends on the signal's last sample, one that starts on its first
add("sd_fbank_packed_f32", "mixed-routes", _fbank_packed(90000, [(0, 640), (100, 32100), (117, 32102), (4000, 9600), (90000 - 48000, 48000), (90000 - 801, 801)]))
add("sd_fbank_packed_f32", "one-launch-only", _fbank_packed(40000, [(39360, 640), (0, 3203), (1000, 16001), (40000 - 32000, 32000)]))
add("sd_fbank_packed_f32", "folded-only", _fbank_packed(70000, [(0, 35003), (70000 - 35003, 35003), (20000, 32160)]))


def test_fbank_workspace_never_shrinks(dev):
    """sd_fbank_workspace_bytes needs a plan (device tables), so its monotonicity in B and n is checked here."""
    lib = N.load()
    for kind, sr in (("speechbrain", 16000), ("torchaudio", 16000), ("torchaudio", 8000), ("torchaudio", 48000)):
        h = _plan(kind, sr).handle
        for n in (640, 16000, 32100, 32160, 48000):
            sizes = [int(lib.sd_fbank_workspace_bytes(h, B, n)) for B in range(1, 601)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (kind, sr, n)
        for B in (1, 31, 256, 257):
            sizes = [int(lib.sd_fbank_workspace_bytes(h, B, n)) for n in range(640, 60000, 79)]
            assert all(b >= a for a, b in zip(sizes, sizes[1:])), (kind, sr, B)
    h = _plan("speechbrain").handle
    for B in (1, 31, 257):
        sizes = [int(lib.sd_fbank_packed_workspace_bytes(h, B, M, 48000)) for M in range(5 * B, 5 * B + 4000, 13)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), B


def test_one_byte_less_of_workspace_is_refused(dev):
    """The sizes of the table above are not generous: told one byte less than the sizing function reports, an entry refuses before it
    launches (the buffer itself stays full size), its output keeps the poison and the guards stay intact.  (The forwards check this in
    every case; sd_seg_gemm_f32 documents a fall-back to the plain operator instead, tests/test_gpu_ops.py.)"""
    from speech_diarization_amd.engine import span_frame_offsets
    lib = N.load()
    A = Arena(dev, 0x7B)
    refused = []

    def expect(name, status, out):
        torch.cuda.synchronize()
        assert status in (SD_ERR_WORKSPACE, -1), (name, status)
        assert bool((out.payload == 0x7B).all()), f"{name}: a refused call wrote to its output"
        refused.append(name)
    plan = _plan("speechbrain")
    for n in (32000, 35003):
        need = int(lib.sd_fbank_workspace_bytes(plan.handle, 3, n))
        if need:
            T = plan.frames(n)
            out = A.scratch(3 * T * 80 * 4, "out")
            expect("sd_fbank_f32", call("sd_fbank_f32", plan.handle, A.data(_wav(1, 3, n), "wav"), 3, n, 1, out, 80, A.scratch(need, "ws"), need - 1), out)
    lens = [640, 35003, 9600]
    fs = span_frame_offsets(lens)
    need = int(lib.sd_fbank_packed_workspace_bytes(plan.handle, 3, int(fs[-1]), max(lens)))
    out = A.scratch(int(fs[-1]) * 80 * 4, "out")
    st = lib.sd_fbank_packed_f32(plan.handle, A.data(_wav(2, 1, 50000)[0], "signal").ptr, 50000, A.data(torch.tensor([0, 100, 40000], dtype=I64), "starts").ptr,
                                 A.data(torch.tensor(lens, dtype=I32), "lens").ptr, A.data(torch.from_numpy(fs), "frame_start").ptr, 3, int(fs[-1]), max(lens),
                                 out.ptr, 80, A.scratch(need, "ws").ptr, need - 1, _stream())
    expect("sd_fbank_packed_f32", st, out)
    n, d = 129, 50
    x = A.data(torch.randn(n, d), "x")
    for entry, size in (("sd_cosine_affinity_f32", lib.sd_cosine_workspace_bytes), ("sd_cosine_affinity_rows_f32", lib.sd_cosine_workspace_bytes),
                        ("sd_cosine_affinity_rows_split16", lib.sd_cosine_split16_workspace_bytes)):
        need = int(size(n, d))
        out = A.scratch(n * n * 4, "out")
        rows = () if entry == "sd_cosine_affinity_f32" else (0, n)
        expect(entry, call(entry, x, n, d, *rows, out, n, A.scratch(need, "ws"), need - 1), out)
    T, K = 257, 8
    need = int(lib.sd_viterbi_workspace_bytes(T, K))
    path = A.scratch(T * 4, "path")
    expect("sd_viterbi_f32", call("sd_viterbi_f32", A.data(torch.randn(T, K), "scores"), K, T, K, -0.1, -3.0, A.scratch(need, "ws"), need - 1, path), path)
    need = int(lib.sd_res2net_chain_workspace_bytes(7))
    r = A.scratch(10 * 1024 * 2, "r")
    layers = (N.sd_layer * 7)()
    expect("sd_res2net_chain_f16", lib.sd_res2net_chain_f16(r.ptr, 1024, 2, 5, layers, 7, A.scratch(need, "ws").ptr, need - 1, _stream()), r)
    assert {"sd_fbank_f32", "sd_fbank_packed_f32", "sd_cosine_affinity_f32", "sd_viterbi_f32", "sd_res2net_chain_f16"} <= set(refused)
    A.check()


# ====================================================================== 1. whole forwards at exactly the reported workspace

_ENGINES = {}


def _geometry(name):
    from speech_diarization_amd.synth import EcapaConfig
    return {"default": EcapaConfig(),
            "c512": EcapaConfig(channels=(512, 512, 512, 512, 1536), attention_channels=128, se_channels=128),
            "small64": EcapaConfig.small(64), "small128": EcapaConfig.small(128)}[name]


def _state(geom):
    from speech_diarization_amd import synth
    if ("sd", geom) not in _ENGINES:
        _ENGINES[("sd", geom)] = synth.make_ecapa_state_dict(1234, _geometry(geom))
    return _ENGINES[("sd", geom)]


def _engine(dev, geom, prec, max_batch=512):
    from speech_diarization_amd.engine import EmbeddingEngine
    key = (geom, prec, max_batch)
    if key not in _ENGINES:
        if max_batch != 512 and (geom, prec, 512) in _ENGINES:             # the same packed weights
            e = _ENGINES[(geom, prec, 512)].sibling()
            e.max_batch = max_batch
            _ENGINES[key] = e
        else:
            _ENGINES[key] = EmbeddingEngine(_state(geom), dev, max_batch=max_batch, precision=prec)
    return _ENGINES[key]


def _fresh(dev, geom, prec, max_batch=512):
    """An engine with a workspace of its own that nothing has run in (the packed weights are shared, read-only)."""
    e = _engine(dev, geom, prec).sibling()
    e.max_batch = max_batch
    return e


def _segments(seed, B, n):
    from speech_diarization_amd import synth
    return torch.from_numpy(synth.synthetic_segments(seed, B, n))


def _entry_of(prec, lens):
    return f"sd_ecapa_forward_{'lens_' if lens else ''}{'f16' if prec == 'f16' else 'f32'}"


def _forward(geom, prec, B, T, lens=False, oracle=False, sel=None):
    """feats exactly [B*T][n_mels], emb exactly [B][dim], the workspace exactly sd_ecapa_workspace_bytes and poisoned.  Equal, bit for
    bit, to `EmbeddingEngine.embed` of the same waveforms (same library, same kernels: that path's parity with the float64 oracle is
    what the rest of the suite establishes); one byte less of workspace is refused with SD_ERR_WORKSPACE and nothing is written."""
    entry = _entry_of(prec, lens)

    def run(dev):
        from speech_diarization_amd.engine import fbank_device
        lib = N.load()
        eng = _engine(dev, geom, prec)
        W = C.byref(eng.weights.struct)
        n = (T - 1) * 160 + (37 if T % 2 else 0)
        wav = _segments(B * 1000 + T, B, n).to(dev)
        rel = _rel_for(B, T).to(dev) if lens else None
        nm, dim = eng.weights.cfg.input_size, eng.dim
        with selection(None, sel):
            if lens:
                feats = torch.empty(B, T, nm, device=dev)
                fws = torch.empty(max(eng.plan.workspace_bytes(B, n), 256), dtype=U8, device=dev)
                ok("sd_fbank_lens_f32", eng.plan.handle, wav, B, n, rel, feats, nm, fws, fws.numel())
            else:
                feats = fbank_device(wav, eng.plan, mean_norm=True)
            need = int(lib.sd_ecapa_workspace_bytes(W, B, T))

            def one(A):
                f_g, ws = A.data(feats, "feats"), A.scratch(need, "workspace")
                emb = A.scratch(B * dim * 4, "emb")
                args = (W, f_g.ptr, B, T) + ((A.data(rel, "rel_len").ptr,) if lens else ()) + (emb.ptr, ws.ptr)
                st = call(entry, *args, need - 1)
                torch.cuda.synchronize()
                assert st == SD_ERR_WORKSPACE, (st, N.last_error())
                assert bool((emb.payload == A.poison).all()), "a refused call wrote to emb"
                G.assert_guards_intact(*A.bufs)
                ok(entry, *args, need)
                return {"emb": emb.view(F32, B, dim)}
            got = under_poisons(dev, one)["emb"]                             # (finite under lengths too: every row of _rel_for keeps a frame)
            want = eng.embed(wav, rel).cpu()
        assert torch.equal(got, want), f"raw ABI vs EmbeddingEngine.embed: {int((got != want).sum())} of {got.numel()} values differ"
        if oracle:
            from oracle import pipeline_ref
            ref = pipeline_ref.encode_batch_ref(_state(geom), wav.cpu().numpy(), torch.float64)
            cd = _cos_dist(got.numpy(), ref)
            assert cd.max() < BAR[prec], cd
    return run


def _forward_packed(geom, T_list, oracle=False, sel=None):
    def run(dev):
        from speech_diarization_amd.engine import fbank_packed_device, span_frame_offsets
        lib = N.load()
        eng = _engine(dev, geom, "f32")
        W = C.byref(eng.weights.struct)
        lens = [(t - 1) * 160 + (11 if t % 2 else 0) for t in T_list]
        B = len(lens)
        starts, at = [], 0
        for i, n in enumerate(lens):                                         # overlapping spans of one signal
            starts.append(at)
            at += n // 2 + 17
        n_total = max(s + n for s, n in zip(starts, lens))
        sig = _segments(B + sum(T_list), 1, n_total)[0].to(dev)
        fs = span_frame_offsets(lens)
        M, dim = int(fs[-1]), eng.dim
        assert fs.tolist() == np.concatenate([[0], np.cumsum(T_list)]).tolist()
        with selection(None, sel):
            feats = fbank_packed_device(sig, starts, lens, eng.plan)
            need = int(lib.sd_ecapa_packed_workspace_bytes(W, B, M))

            def one(A):
                f_g, fs_g, ws = A.data(feats, "feats"), A.data(torch.from_numpy(fs), "frame_start"), A.scratch(need, "workspace")
                emb = A.scratch(B * dim * 4, "emb")
                st = call("sd_ecapa_forward_packed_f32", W, f_g, fs_g, B, M, emb, ws, need - 1)
                torch.cuda.synchronize()
                assert st == SD_ERR_WORKSPACE and bool((emb.payload == A.poison).all())
                ok("sd_ecapa_forward_packed_f32", W, f_g, fs_g, B, M, emb, ws, need)
                return {"emb": emb.view(F32, B, dim)}
            got = under_poisons(dev, one)["emb"]
            want = eng.embed_spans(sig, np.asarray(starts), np.asarray(lens), frame_budget=M).cpu()
        assert torch.equal(got, want)
        if oracle:
            from oracle import pipeline_ref
            s = sig.cpu().numpy()
            ref = np.concatenate([pipeline_ref.encode_batch_ref(_state(geom), s[None, a:a + n]) for a, n in zip(starts, lens)])
            assert _cos_dist(got.numpy(), ref).max() < BAR["f32"]
    return run


def _threshold_shapes():
    """(B, T): both sides of every threshold of the schedule, each once -- B: 1, 31, 224 | 225, 255 | 256 | 257 (the split-K scratch exists up
    to 256 rows; it was once short at 225 .. 256); T: 5 (the floor), 63 | 64 and 127 | 128 (column statistics switch on), 201 (the
    benchmark's shape), the last T the fused Res2Net chain and the fused pooling accept and the first they refuse (asked of the
    library), 3001 with a small B; and three (B, T) whose product is a multiple of no tile height."""
    c_last, c_first = _chain_T_limits()
    a_last, a_first = _asp_T_limits()
    return [(1, 5), (31, 201), (224, 63), (225, 64), (255, 127), (256, 128), (257, c_last), (3, c_first), (2, a_last), (2, a_first), (2, 3001),
            (37, 7), (29, 9), (19, 17)]


def test_threshold_shapes_cover_both_sides():
    lib = N.load()
    assert {1, 31, 224, 225, 255, 256, 257} <= {B for B, _ in _SHAPES}
    c_last, c_first = _chain_T_limits()
    a_last, a_first = _asp_T_limits()
    assert lib.sd_res2net_chain_supported(c_last, 128, 7, 3, 4) and not lib.sd_res2net_chain_supported(c_first, 128, 7, 3, 4)
    for dt in (N.SD_DT_F32, N.SD_DT_F16):
        assert lib.sd_asp_attend_pool_supported(dt, a_last, 3072, 128) and not lib.sd_asp_attend_pool_supported(dt, a_first, 3072, 128)
    assert {5, 63, 64, 127, 128, 201, c_last, c_first, a_last, a_first, 3001} <= {T for _, T in _SHAPES}
    for B, T in _SHAPES[-3:]:
        assert all((B * T) % h for h in TILE_ROWS)


# (the two fused kernels' length limits are asked of the library -- host code, no device -- when the table is built)
_SHAPES = _threshold_shapes()
_C512_SHAPES = [(1, 5), (31, 201), (256, 64), (257, 128), (5, _chain_T_limits()[0]), (5, _chain_T_limits()[1]), (3, _asp_T_limits()[1]), (37, 7)]
_SMALL_SHAPES = [(31, 5), (257, 64), (2, 201), (19, 17)]
_LENS_SHAPES = {"default": [(31, 201), (225, 5), (256, 64), (257, 128), (3, _chain_T_limits()[1])], "c512": [(7, 128), (37, 7), (3, _asp_T_limits()[1])],
                "small128": [(31, 5)]}

for _prec in ("f32", "f32s", "f32ns", "f16"):
    _e = _entry_of(_prec, False)
    for _B, _T in _SHAPES:
        add(_e, f"default-{_prec}-B{_B}-T{_T}", _forward("default", _prec, _B, _T, oracle=(_B, _T) == _SHAPES[7]))
    for _B, _T in _C512_SHAPES:
        add(_e, f"c512-{_prec}-B{_B}-T{_T}", _forward("c512", _prec, _B, _T))
    for _g in ("small64", "small128"):
        for _B, _T in _SMALL_SHAPES:
            add(_e, f"{_g}-{_prec}-B{_B}-T{_T}", _forward(_g, _prec, _B, _T))
    for _g, _lst in _LENS_SHAPES.items():
        for _B, _T in _lst:
            add(_entry_of(_prec, True), f"{_g}-{_prec}-B{_B}-T{_T}", _forward(_g, _prec, _B, _T, lens=True))
for _sel in CONV_KERNELS:
    add("sd_ecapa_forward_f32", f"default-f32-B31-T201-{_sel}", _forward("default", "f32", 31, 201, sel=_sel))
    add("sd_ecapa_forward_f32", f"default-f32-B37-T7-{_sel}", _forward("default", "f32", 37, 7, sel=_sel))
    add("sd_ecapa_forward_f32", f"c512-f32-B5-T129-{_sel}", _forward("c512", "f32", 5, 129, sel=_sel))

_SPANS = {
    "one-5-frame-span": [5],
    "B31-mixed": [5, 201, 7, 63, 64, 9, 128, 5, 17, 127, 213, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 257, 5, 33, 101],
    "B256-short": [5 + (i % 5) for i in range(256)],
    "B257-short": [5 + (i % 7) for i in range(257)],
    "B225": [5 + (i % 3) for i in range(225)],
    "T3001": [5, 3001, 201],
}
for _name, _T_list in _SPANS.items():
    add("sd_ecapa_forward_packed_f32", f"default-{_name}", _forward_packed("default", _T_list, oracle=_name == "T3001"))
for _g in ("c512", "small64", "small128"):
    add("sd_ecapa_forward_packed_f32", f"{_g}-B31-mixed", _forward_packed(_g, _SPANS["B31-mixed"]))
    add("sd_ecapa_forward_packed_f32", f"{_g}-B257-short", _forward_packed(_g, _SPANS["B257-short"]))
for _sel in CONV_KERNELS:
    add("sd_ecapa_forward_packed_f32", f"default-B31-mixed-{_sel}", _forward_packed("default", _SPANS["B31-mixed"], sel=_sel))


# ====================================================================== the table, run

@pytest.mark.parametrize("entry,cid", [(e, cid) for e in CASES for cid, _ in CASES[e]])
def test_guarded(dev, entry, cid):
    fn = dict(CASES[entry])[cid]
    with torch.cuda.device(dev):
        fn(dev)


# ====================================================================== the product-level form: one engine, one growing workspace

def _spans_of(n_total, lens):
    starts, at = [], 0
    for n in lens:
        starts.append(at)
        at = min(at + n // 3 + 5, n_total - max(lens))
    return np.asarray(starts), np.asarray(lens)


@pytest.mark.parametrize("prec", ["f32", "f32s", "f32ns", "f16"])
def test_one_engine_serves_a_sequence_of_calls_as_fresh_engines_would(dev, prec):
    """The workspace only ever grows and is reused across batch sizes, lengths and the uniform / lens / packed schedules, so stale
    contents are the normal case: a large batch with a short last micro-batch, a short small batch, a lens batch, packed spans (f32),
    the small batch again -- each bitwise the result of a fresh engine given only that call.  The same through a sibling()."""
    geom = "c512"
    max_batch = 48
    one = _fresh(dev, geom, prec, max_batch)
    big = _segments(1, 2 * max_batch + 7, 48000).to(dev)                     # T = 301: the unfused pooling, three micro-batches (48, 48, 7)
    small = _segments(2, 5, 3200).to(dev)                                    # T = 21
    ragged = _segments(3, 9, 20320).to(dev)                                  # T = 128
    rel = _rel_for(9, 128).to(dev)
    sig = _segments(4, 1, 90000)[0].to(dev)
    st, ln = _spans_of(90000, [640, 32000, 1600, 48000, 9600, 800])
    calls = [("big", lambda e: e.embed(big)), ("small", lambda e: e.embed(small)), ("lens", lambda e: e.embed(ragged, rel))]
    if prec == "f32":
        calls.append(("spans", lambda e: e.embed_spans(sig, st, ln)))
    calls += [("windows", lambda e: e.embed_windows(sig, torch.tensor([0, 500, 89000, -200, 40000]), 16000)), ("small again", lambda e: e.embed(small))]
    for engine in (one, one.sibling()):
        for name, f in calls:
            got = f(engine).cpu()
            want = f(_fresh(dev, geom, prec, max_batch)).cpu()
            assert bool(torch.isfinite(got).all()) and torch.equal(got, want), (prec, name)


def test_encode_batches_with_two_in_flight_equals_the_batches_alone(dev):
    from speech_diarization_amd.speech_encode import HipEcapaEncoder
    enc = HipEcapaEncoder(_state("c512"), dev, max_batch=48)
    batches = [_segments(10 + i, B, n) for i, (B, n) in enumerate([(55, 32000), (5, 3200), (48, 16000), (7, 48000), (5, 3200), (49, 640)])]
    got = enc.encode_batches(batches, lanes=2)
    for b, g in zip(batches, got):
        alone = HipEcapaEncoder(_state("c512"), dev, max_batch=48).encode_batch(b)
        g, alone = torch.as_tensor(np.asarray(g)).reshape(b.shape[0], -1), torch.as_tensor(np.asarray(alone.cpu())).reshape(b.shape[0], -1)
        assert torch.equal(g, alone)


@pytest.mark.parametrize("prec,T", [("f32", 5), ("f16", 201)])
def test_max_batch_257_serves_its_256_row_remainder(dev, prec, T):
    """sd_ecapa_workspace_bytes used to shrink from 256 to 257 rows (the split-K scratch was reserved up to 256 rows only), and the engine
    runs its last micro-batch in the workspace sized for the first: with max_batch = 257 and 513 segments the 256-row remainder was
    refused with SD_ERR_WORKSPACE on a fresh engine.  Default geometry; bitwise two separate calls."""
    n = (T - 1) * 160
    wav = _segments(T, 513, n).to(dev)
    got = _fresh(dev, "default", prec, 257).embed(wav)
    first = _fresh(dev, "default", prec, 512).embed(wav[:257])
    last = _fresh(dev, "default", prec, 512).embed(wav[257:])
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got[:257], first) and torch.equal(got[257:], last)
