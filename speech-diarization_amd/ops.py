"""Thin torch-tensor wrappers over the layer / cosine operators of libsd_hip.so.

Inputs and outputs are CUDA tensors; every call is asynchronous on the current
torch stream.  These are the operators `sd_ecapa_forward_f32` is built from, exposed
so that each can be parity-tested on its own, plus the cosine helpers used by the
clustering-side callers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _native as N

_ACT = {None: N.SD_ACT_NONE, "none": N.SD_ACT_NONE, "relu": N.SD_ACT_RELU, "tanh": N.SD_ACT_TANH, "sigmoid": N.SD_ACT_SIGMOID}


_ENTRIES = frozenset(name for key, table in vars(N).items() if key.endswith("PROTOTYPES") for name in table)
_LAUNCHABLE = _ENTRIES | frozenset(N.TREE_ENTRIES)      # what `launch` accepts: the six *_PROTOTYPES tables and the table of sd_hip_tree.h
_CUT_LAUNCHABLE = frozenset(N.CUT_ENTRIES)              # ... and, in a set of its own, the table of sd_hip_cut.h
_KMEANS_LAUNCHABLE = frozenset(N.KMEANS_ENTRIES)        # ... and the table of sd_hip_kmeans.h
_VAD_LAUNCHABLE = frozenset(N.VAD_ENTRIES)              # ... and the table of sd_hip_vad.h
_SCD_LAUNCHABLE = frozenset(N.SCD_ENTRIES)              # ... and the table of sd_hip_scd.h
_TURNS_LAUNCHABLE = frozenset(N.TURNS_ENTRIES)          # ... and the table of sd_hip_turns.h


def _current_stream(index: int) -> int:
    """The raw handle of the current torch stream of GPU `index`: the one place the binding asks torch for it."""
    return torch.cuda.current_stream(index).cuda_stream


def _stream(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(_current_stream(t.device.index))


def launch(name: str, on: torch.Tensor, *args) -> None:
    """The one checked launch of the binding: entry `name` of the C ABI on the device of `on`, `args` followed by the current stream
    of that device (every launching entry takes its stream last), a non-zero status raised as `SdError` under the same `name`."""
    if (name not in _LAUNCHABLE and name not in _CUT_LAUNCHABLE and name not in _KMEANS_LAUNCHABLE and name not in _VAD_LAUNCHABLE
            and name not in _SCD_LAUNCHABLE and name not in _TURNS_LAUNCHABLE):
        raise ValueError(f"{name!r} is in none of the prototype tables of _native: not an entry of libsd_hip.so")
    with torch.cuda.device(on.device.index):            # by index: this runs once per launch, and torch resolves an int at once
        N.check(getattr(N.load(), name)(*args, _stream(on)), name)


class Workspace:
    """A grow-only uint8 buffer on one device, for the entries that take a workspace: kept between calls, it is allocated again only
    when a call needs more than it holds."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.buf = None

    def take(self, need: int) -> torch.Tensor:
        """At least max(need, 16) bytes; the same storage as the last call unless `need` exceeds it."""
        if self.buf is None or self.buf.numel() < need:
            self.buf = torch.empty((max(need, 16),), dtype=torch.uint8, device=self.device)
        return self.buf


def _need_cuda(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is not None and t.device.type != "cuda":
            raise RuntimeError("libsd_hip operators take GPU tensors; there is no CPU fallback")


def _ptr(t):
    return None if t is None else t.data_ptr()


def pack_weight(w: torch.Tensor | np.ndarray, device, dtype=torch.float32) -> torch.Tensor:
    """[cout, cin, k] -> packed [cout, k, cin_pad] on `device` (f32: cin_pad % 32 == 0, f16: % 64)."""
    from .engine import pack_conv_weight
    w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
    npdt = np.float16 if dtype == torch.float16 else np.float32
    return torch.from_numpy(pack_conv_weight(w.astype(np.float32), npdt)).to(device)


def _dt(t: torch.dtype) -> int:
    if t == torch.float32:
        return N.SD_DT_F32
    if t == torch.float16:
        return N.SD_DT_F16
    raise TypeError(f"unsupported dtype {t}")


def _conv_args(x: int, lda: int, a_col0: int, x_dtype: int, w: int, w_dtype: int, y: int, ldo: int, o_col0: int, y_dtype: int, M: int, T: int,
               cin: int, cin_pad: int, cout: int, taps: int, dil: int, *, bias=None, bias_per_seg=False, act=None, act2=None, scale=None, shift=None,
               tee=None, tee_lo: int = 0, tee_hi: int = 0, tee_add=None, ta_col0: int = 0, colstat=None) -> N.sd_conv_args:
    """One `sd_conv_args` (x / w / y: device pointers; the optional vectors and buffers: tensors or None)."""
    a = N.sd_conv_args()
    a.x, a.lda, a.a_col0, a.x_dtype = x, lda, a_col0, x_dtype
    a.w, a.w_dtype = w, w_dtype
    a.y, a.ldo, a.o_col0, a.y_dtype = y, ldo, o_col0, y_dtype
    a.M, a.T = M, T
    a.cin, a.cin_pad, a.cout, a.taps, a.dil = cin, cin_pad, cout, taps, dil
    a.bias, a.bias_per_seg = _ptr(bias), int(bool(bias_per_seg))
    a.act, a.act2 = _ACT[act], _ACT[act2]
    a.scale, a.shift = _ptr(scale), _ptr(shift)
    if tee is not None:
        a.tee, a.ldt, a.tee_lo, a.tee_hi = tee.data_ptr(), tee.stride(0), tee_lo, tee_hi
        if tee_add is not None:
            a.tee_add, a.ld_ta, a.ta_col0 = tee_add.data_ptr(), tee_add.stride(0), ta_col0
    if colstat is not None:
        a.colstat = colstat.data_ptr()
    return a


def conv1d_cl(x: torch.Tensor, w_packed: torch.Tensor, T: int, *, cin: int, dil: int = 1, bias=None, bias_per_seg=False,
              act=None, scale=None, shift=None, act2=None, a_col0: int = 0, out: torch.Tensor | None = None,
              o_col0: int = 0, tee: torch.Tensor | None = None, tee_lo: int = 0, tee_hi: int = 0,
              tee_add: torch.Tensor | None = None, ta_col0: int = 0, out_dtype: torch.dtype | None = None,
              colstat: torch.Tensor | None = None) -> torch.Tensor:
    """Channel-last conv1d ("same", reflect) with the fused TDNN epilogue. x: [M, lda], returns [M, ldo].
    f32 weights -> exact-f32 operator; f16 weights -> f16-operand / f32-accumulate operator (x f32 or
    f16, output `out_dtype`).  `colstat` (f32, `colstat_floats(M, cout)` elements) receives the epilogue's
    per-tile column sums for `colstat_finish`."""
    _need_cuda(x, w_packed, bias, scale, shift, out, tee, tee_add, colstat)
    cout, taps, cin_pad = w_packed.shape
    M = x.shape[0]
    half = w_packed.dtype == torch.float16
    if out is None:
        out = torch.empty((M, cout), dtype=out_dtype or (torch.float16 if half else torch.float32), device=x.device)
    for extra in (tee, tee_add):
        if extra is not None and extra.dtype != out.dtype:
            raise TypeError("tee / tee_add must have the output dtype")
    if colstat is not None and (colstat.dtype != torch.float32 or colstat.numel() < colstat_floats(M, cout)):
        raise ValueError("colstat must be f32 with colstat_floats(M, cout) elements")
    a = _conv_args(x.data_ptr(), x.stride(0), a_col0, _dt(x.dtype), w_packed.data_ptr(), _dt(w_packed.dtype), out.data_ptr(), out.stride(0), o_col0,
                   _dt(out.dtype), M, T, cin, cin_pad, cout, taps, dil, bias=bias, bias_per_seg=bias_per_seg, act=act, act2=act2, scale=scale,
                   shift=shift, tee=tee, tee_lo=tee_lo, tee_hi=tee_hi, tee_add=tee_add, ta_col0=ta_col0, colstat=colstat)
    launch("sd_conv1d_cl_f16" if half else "sd_conv1d_cl_f32", x, C.byref(a))
    return out


def _span_table(frame_start, device) -> tuple[torch.Tensor, int]:
    fs = frame_start.to(device, dtype=torch.int32).contiguous() if isinstance(frame_start, torch.Tensor) else \
        torch.from_numpy(np.ascontiguousarray(frame_start, dtype=np.int32)).to(device)
    return fs, int(fs.numel()) - 1


def conv1d_cl_packed(x: torch.Tensor, w_packed: torch.Tensor, frame_start, *, cin: int, dil: int = 1, bias=None, bias_per_seg=False,
                     act=None, scale=None, shift=None, act2=None, a_col0: int = 0, out: torch.Tensor | None = None, o_col0: int = 0,
                     tee: torch.Tensor | None = None, tee_lo: int = 0, tee_hi: int = 0, tee_add: torch.Tensor | None = None,
                     ta_col0: int = 0) -> torch.Tensor:
    """`conv1d_cl` (exact f32) over packed spans: rows frame_start[s] .. frame_start[s + 1] of x are span s, the reflect padding and a
    per-segment bias (bias [B, cout]) are the span's (`sd_conv1d_cl_packed_f32`)."""
    _need_cuda(x, w_packed, bias, scale, shift, out, tee, tee_add)
    cout, taps, cin_pad = w_packed.shape
    M = x.shape[0]
    fs, B = _span_table(frame_start, x.device)
    if out is None:
        out = torch.empty((M, cout), dtype=torch.float32, device=x.device)
    a = _conv_args(x.data_ptr(), x.stride(0), a_col0, _dt(x.dtype), w_packed.data_ptr(), _dt(w_packed.dtype), out.data_ptr(), out.stride(0), o_col0,
                   _dt(out.dtype), M, M, cin, cin_pad, cout, taps, dil, bias=bias, bias_per_seg=bias_per_seg, act=act, act2=act2, scale=scale,
                   shift=shift, tee=tee, tee_lo=tee_lo, tee_hi=tee_hi, tee_add=tee_add, ta_col0=ta_col0)
    launch("sd_conv1d_cl_packed_f32", x, C.byref(a), fs.data_ptr(), B)
    return out


def seg_mean_std_packed(x: torch.Tensor, frame_start, want_std: bool = True, eps: float = 1e-12) -> torch.Tensor:
    """Per-span mean (and std) of x [M, C] over rows frame_start[s] .. frame_start[s + 1] -> f32 [B, C] or [B, 2C]."""
    _need_cuda(x)
    fs, B = _span_table(frame_start, x.device)
    C_ = x.shape[1]
    out = torch.empty((B, (2 if want_std else 1) * C_), dtype=torch.float32, device=x.device)
    launch("sd_seg_mean_std_packed_dt", x, x.data_ptr(), _dt(x.dtype), x.stride(0), 0, fs.data_ptr(), B, x.shape[0], C_, int(bool(want_std)),
           C.c_float(eps), out.data_ptr())
    return out


def se_scale_residual_packed(x: torch.Tensor, gate: torch.Tensor, res: torch.Tensor, frame_start) -> torch.Tensor:
    """y[m] = x[m] * gate[span of m] + res[m] over packed spans."""
    _need_cuda(x, gate, res)
    fs, B = _span_table(frame_start, x.device)
    y = torch.empty_like(x)
    launch("sd_se_scale_residual_packed_dt", x, x.data_ptr(), x.stride(0), gate.data_ptr(), res.data_ptr(), res.stride(0), 0, y.data_ptr(),
           y.stride(0), 0, fs.data_ptr(), B, x.shape[0], x.shape[1], _dt(x.dtype))
    return y


def asp_pool_packed(logit: torch.Tensor, h: torch.Tensor, frame_start, eps: float = 1e-12) -> torch.Tensor:
    """Attentive statistics pooling (softmax over each span's rows) over packed spans -> f32 [B, 2C]."""
    _need_cuda(logit, h)
    fs, B = _span_table(frame_start, h.device)
    C_ = h.shape[1]
    out = torch.empty((B, 2 * C_), dtype=torch.float32, device=h.device)
    launch("sd_asp_pool_packed_dt", h, logit.data_ptr(), logit.stride(0), h.data_ptr(), _dt(h.dtype), h.stride(0), fs.data_ptr(), B, h.shape[0], C_,
           C.c_float(eps), out.data_ptr())
    return out


def seg_gemm(x: torch.Tensor, w_packed: torch.Tensor, *, cin: int, bias=None, act=None, scale=None, shift=None, act2=None,
             out: torch.Tensor | None = None, scratch: torch.Tensor | None = None) -> torch.Tensor:
    """A per-segment layer (one row per segment: SE squeeze FC, global-context bias, final FC) through `sd_seg_gemm_f32`: with `scratch`
    (f32, `seg_gemm_scratch_bytes` bytes; allocated here when None) K is split over the grid for M <= 256 rows and cin_pad >= 512."""
    _need_cuda(x, w_packed, bias, scale, shift, out, scratch)
    lib = N.load()
    cout, taps, cin_pad = w_packed.shape
    M = x.shape[0]
    if taps != 1 or w_packed.dtype != torch.float32 or x.dtype != torch.float32:
        raise TypeError("seg_gemm: f32 activations and one-tap f32 weights")
    if out is None:
        out = torch.empty((M, cout), dtype=torch.float32, device=x.device)
    need = int(lib.sd_seg_gemm_scratch_bytes(M, cin_pad, cout))
    if scratch is None and need:
        scratch = torch.empty(need // 4, dtype=torch.float32, device=x.device)
    a = _conv_args(x.data_ptr(), x.stride(0), 0, N.SD_DT_F32, w_packed.data_ptr(), N.SD_DT_F32, out.data_ptr(), out.stride(0), 0, N.SD_DT_F32,
                   M, 1, cin, cin_pad, cout, 1, 1, bias=bias, act=act, act2=act2, scale=scale, shift=shift)
    launch("sd_seg_gemm_f32", x, C.byref(a), _ptr(scratch), scratch.numel() * 4 if scratch is not None else 0)
    return out


def split16_pack(x: torch.Tensor, a_col0: int = 0, cin: int | None = None, mul: float = 1.0) -> torch.Tensor:
    """f32 [M, ld] columns [a_col0, a_col0 + cin) -> SD_DT_SPLIT16 rows as an f16 tensor [M, 2 * cin_pad32]
    (per 32 values: [hi x 32 | lo x 32], hi = f16(v), lo = f16(v - hi); padding values zero)."""
    _need_cuda(x)
    if x.dtype != torch.float32 or x.stride(1) != 1:
        raise TypeError("x must be f32 with contiguous channels")
    M = x.shape[0]
    cin = x.shape[1] - a_col0 if cin is None else cin
    cp = (cin + 31) // 32 * 32
    out = torch.empty((M, 2 * cp), dtype=torch.float16, device=x.device)
    launch("sd_split16_pack_f32", x, x.data_ptr(), x.stride(0), a_col0, M, cin, C.c_float(mul), out.data_ptr(), cp)
    return out


def pack_weight_split16(w: torch.Tensor | np.ndarray, device):
    """[cout, cin, k] -> (SD_DT_SPLIT16 weights as an f16 tensor [cout, k, cin_pad32 / 32, 64] on `device`, s):
    scaled by 2^s, hi / lo halves interleaved per 32 input channels (`engine.pack_conv_weight_split16`)."""
    from .engine import pack_conv_weight_split16
    w = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
    packed, s = pack_conv_weight_split16(w.astype(np.float32))
    return torch.from_numpy(packed).to(device), s


def conv1d_cl_split16(x: torch.Tensor, w_split: torch.Tensor, w_shift: int, T: int, *, cin: int, dil: int = 1, bias=None, bias_per_seg=False,
                      act=None, scale=None, shift=None, act2=None, a_col0: int = 0, out: torch.Tensor | None = None, o_col0: int = 0,
                      tee: torch.Tensor | None = None, tee_lo: int = 0, tee_hi: int = 0, tee_add: torch.Tensor | None = None, ta_col0: int = 0,
                      colstat: torch.Tensor | None = None, narrow: bool = False, out_split: torch.Tensor | None = None) -> torch.Tensor:
    """The "f32-split16x3" conv: f32 x [M, lda] -> f32 y [M, ldo] at f32-level accuracy on the f16 matrix cores.
    `w_split`, `w_shift` from `pack_weight_split16`; bias / scale / shift are the layer's ordinary f32 vectors.
    Default (wide outputs): `sd_split16_pack_f32` + the 256x256 kernel, the 2^s of the weight scaling folded into bias and scale here.
    `narrow=True`: the 128x128 kernel that splits the f32 activations while staging them (no pack pass; tee_add, per-segment bias and
    act2 allowed, no colstat), the 2^-s passed as `w_scale_inv`; `out_split`: its y as SD_DT_SPLIT16 rows instead of f32."""
    _need_cuda(x, w_split, bias, scale, shift, out, tee, tee_add, colstat)
    cout, taps, chunks, _ = w_split.shape
    cp = chunks * 32
    M = x.shape[0]
    if out is None:
        out = torch.empty((M, cout), dtype=torch.float32, device=x.device)
    f = float(2.0 ** w_shift)
    if narrow:
        if x.dtype != torch.float32 or x.stride(1) != 1:
            raise TypeError("x must be f32 with contiguous channels")
        keep = (x,)
        xp, lda, xcol, xdt, bias_k, scale_k = x.data_ptr(), x.stride(0), a_col0, N.SD_DT_F32, bias, scale
    else:
        if bias_per_seg or act2 is not None or tee_add is not None:
            raise ValueError("per-segment bias / act2 / tee_add belong to the narrow kernel (narrow=True)")
        xs = split16_pack(x, a_col0, cin)
        bias_k = None if bias is None else bias * f
        scale_k = (torch.full((cout,), 1.0 / f, dtype=torch.float32, device=x.device) if scale is None else scale / f)
        keep = (xs, bias_k, scale_k)
        xp, lda, xcol, xdt = xs.data_ptr(), cp, 0, N.SD_DT_SPLIT16
    yp, ldo, ydt = out.data_ptr(), out.stride(0), N.SD_DT_F32
    if out_split is not None:
        # y leaves as SD_DT_SPLIT16 rows (f16 [M, 2 * ld], ld VALUE columns, a multiple of 32) instead of f32 --
        # bit for bit what split16_pack would make of the f32 result; `out` is then not written
        if out_split.dtype != torch.float16 or out_split.stride(1) != 1 or out_split.shape[1] % 64 or colstat is not None:
            raise TypeError("out_split: f16 [M, 2 * ld] with ld % 32 == 0, no colstat")
        _need_cuda(out_split)
        yp, ldo, ydt = out_split.data_ptr(), out_split.shape[1] // 2, N.SD_DT_SPLIT16
    a = _conv_args(xp, lda, xcol, xdt, w_split.data_ptr(), N.SD_DT_SPLIT16, yp, ldo, o_col0, ydt, M, T, cin, cp, cout, taps, dil, bias=bias_k,
                   bias_per_seg=bias_per_seg, act=act, act2=act2, scale=scale_k, shift=shift, tee=tee, tee_lo=tee_lo, tee_hi=tee_hi, tee_add=tee_add,
                   ta_col0=ta_col0, colstat=colstat)
    if narrow:
        a.w_scale_inv = 1.0 / f
    launch("sd_conv1d_cl_split16", x, C.byref(a))
    del keep
    return out


def res2net_chain_supported(T: int, chunk: int = 128, n: int = 7, taps: int = 3, dil: int = 2) -> bool:
    return bool(N.load().sd_res2net_chain_supported(T, chunk, n, taps, dil))


def res2net_chain(r: torch.Tensor, T: int, layers: list[dict]) -> torch.Tensor:
    """The Res2Net chain of one SE-Res2Net block in one kernel, IN PLACE on the tdnn1 output r [B*T, ld] (f16):
    y_1 = TDNN_1(c_1), y_j = TDNN_j(c_j + y_{j-1}); c_j = columns [128 j, 128 j + 128), y_j overwrites c_j.
    layers[j]: dict(w=packed f16 [128, 3, 128], bias, scale, shift (f32 [128] or None), dil)."""
    _need_cuda(r)
    if r.dtype != torch.float16 or r.stride(1) != 1:
        raise TypeError("r must be f16 with contiguous channels")
    arr = (N.sd_layer * len(layers))()
    for L, d in zip(arr, layers):
        _need_cuda(d["w"], d.get("bias"), d.get("scale"), d.get("shift"))
        cout, taps, cin_pad = d["w"].shape
        L.w, L.bias, L.scale, L.shift = d["w"].data_ptr(), _ptr(d.get("bias")), _ptr(d.get("scale")), _ptr(d.get("shift"))
        L.cin, L.cin_pad, L.cout, L.taps, L.dil, L.w_dtype = d.get("cin", cin_pad), cin_pad, cout, taps, d["dil"], _dt(d["w"].dtype)
    B = r.shape[0] // T
    ws_bytes = max(256, int(N.load().sd_res2net_chain_workspace_bytes(len(layers))))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=r.device)
    launch("sd_res2net_chain_f16", r, r.data_ptr(), r.stride(0), B, T, arr, len(layers), ws.data_ptr(), ws_bytes)
    return r


def colstat_floats(M: int, cout: int) -> int:
    return int(N.load().sd_colstat_floats(M, cout))


def colstat_finish(colstat: torch.Tensor, y: torch.Tensor, B: int, T: int, *, pivot: torch.Tensor | None = None, want_std: bool = False,
                   eps: float = 1e-12, y_col0: int = 0, C_: int | None = None) -> torch.Tensor:
    """Per-segment mean (and std) of a conv output from the column sums its epilogue left in `colstat`
    (`pivot` = the conv's `shift`, or None).  -> f32 [B, C] or [B, 2C] = [mean | std]."""
    _need_cuda(colstat, y, pivot)
    C_ = y.shape[1] - y_col0 if C_ is None else C_
    out = torch.empty((B, (2 if want_std else 1) * C_), dtype=torch.float32, device=y.device)
    launch("sd_colstat_finish_dt", y, colstat.data_ptr(), _ptr(pivot), y.data_ptr(), _dt(y.dtype), y.stride(0), y_col0, B, T, C_, int(want_std),
           C.c_float(eps), out.data_ptr())
    return out


def seg_mean(x: torch.Tensor, B: int, T: int, col0: int = 0, C_: int | None = None) -> torch.Tensor:
    _need_cuda(x)
    C_ = x.shape[1] - col0 if C_ is None else C_
    out = torch.empty((B, C_), dtype=torch.float32, device=x.device)
    launch("sd_seg_mean_f32", x, x.data_ptr(), x.stride(0), col0, B, T, C_, out.data_ptr())
    return out


def seg_mean_std(x: torch.Tensor, B: int, T: int, eps: float = 1e-12) -> torch.Tensor:
    _need_cuda(x)
    C_ = x.shape[1]
    out = torch.empty((B, 2 * C_), dtype=torch.float32, device=x.device)
    launch("sd_seg_mean_std_f32", x, x.data_ptr(), x.stride(0), 0, B, T, C_, C.c_float(eps), out.data_ptr())
    return out


def se_scale_residual(x: torch.Tensor, gate: torch.Tensor, res: torch.Tensor, B: int, T: int) -> torch.Tensor:
    _need_cuda(x, gate, res)
    C_ = x.shape[1]
    y = torch.empty_like(x)
    launch("sd_se_scale_residual_f32", x, x.data_ptr(), x.stride(0), gate.data_ptr(), res.data_ptr(), res.stride(0), 0, y.data_ptr(), y.stride(0), 0,
           B, T, C_)
    return y


def asp_pool(logit: torch.Tensor, h: torch.Tensor, B: int, T: int, eps: float = 1e-12) -> torch.Tensor:
    _need_cuda(logit, h)
    C_ = h.shape[1]
    out = torch.empty((B, 2 * C_), dtype=torch.float32, device=h.device)
    launch("sd_asp_pool_f32", h, logit.data_ptr(), logit.stride(0), h.data_ptr(), h.stride(0), B, T, C_, C.c_float(eps), out.data_ptr())
    return out


def asp_attend_pool(a1: torch.Tensor, wc_packed: torch.Tensor, h: torch.Tensor, B: int, T: int, eps: float = 1e-12, split16: bool = False) -> torch.Tensor:
    """softmax_T(a1 @ wc^T) weighted mean / std of h in one kernel (`asp.conv` + pooling of speechbrain's
    AttentiveStatisticsPooling): a1 [B*T, att], wc_packed from `pack_weight`, h [B*T, C] -> f32 [B, 2C].
    Raises for geometries the fused kernel does not cover (see `asp_attend_pool_supported`)."""
    _need_cuda(a1, h, wc_packed)
    C_, att = h.shape[1], a1.shape[1]
    if a1.dtype != h.dtype or wc_packed.dtype != h.dtype:
        raise ValueError("a1, wc and h must share a dtype")
    dt = N.SD_DT_F16 if h.dtype == torch.float16 else N.SD_DT_F32
    if split16:       # f32 tensors, the logits product as three f16 MFMA products per value pair (the f32-split16x3 mode)
        if h.dtype != torch.float32:
            raise ValueError("split16 takes f32 tensors")
        dt = N.SD_DT_SPLIT16
    a1 = a1.contiguous()
    out = torch.empty((B, 2 * C_), dtype=torch.float32, device=h.device)
    launch("sd_asp_attend_pool_dt", h, a1.data_ptr(), wc_packed.data_ptr(), h.data_ptr(), dt, h.stride(0), B, T, C_, att, C.c_float(eps),
           out.data_ptr())
    return out


def asp_attend_pool_supported(dtype: torch.dtype, T: int, C_: int, att: int) -> bool:
    return bool(N.load().sd_asp_attend_pool_supported(N.SD_DT_F16 if dtype == torch.float16 else N.SD_DT_F32, T, C_, att))


def l2norm_rows(x: torch.Tensor, eps_add: float = 0.0, sklearn_zero_guard: bool = False) -> torch.Tensor:
    _need_cuda(x)
    x = x.contiguous().float()
    n, d = x.shape
    out = torch.empty_like(x)
    launch("sd_l2norm_rows_f32", x, x.data_ptr(), d, n, d, C.c_float(eps_add), int(sklearn_zero_guard), out.data_ptr(), d)
    return out


def cosine_affinity(x: torch.Tensor, out: torch.Tensor | None = None, rows: tuple[int, int] | None = None,
                    split16: bool = False) -> torch.Tensor:
    """sklearn `cosine_similarity(X)` semantics on the GPU: f32 [N, D] -> f32 [N, N]
    (or rows [lo, hi) of it -> [hi-lo, N] when `rows` is given).  `split16`: same result to ~3e-7 through
    the f16 matrix cores (rows split hi + lo), for very large N."""
    _need_cuda(x)
    lib = N.load()
    x = x.contiguous().float()
    n, d = x.shape
    lo, hi = (0, n) if rows is None else rows
    if out is None:
        out = torch.empty((hi - lo, n), dtype=torch.float32, device=x.device)
    if n == 0 or hi == lo:
        return out
    size_fn, name = ((lib.sd_cosine_split16_workspace_bytes, "sd_cosine_affinity_rows_split16") if split16 else
                     (lib.sd_cosine_workspace_bytes, "sd_cosine_affinity_rows_f32"))
    ws_bytes = int(size_fn(n, d))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=x.device)
    launch(name, x, x.data_ptr(), n, d, lo, hi, out.data_ptr(), out.stride(0), ws.data_ptr(), ws_bytes)
    return out


def adjacent_cosine(x: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    _need_cuda(x)
    x = x.contiguous().float()
    n, d = x.shape
    out = torch.empty((max(n - 1, 0),), dtype=torch.float32, device=x.device)
    launch("sd_adjacent_cosine_f32", x, x.data_ptr(), d, n, d, C.c_float(eps), out.data_ptr())
    return out


def sim_argmax(w: torch.Tensor, c: torch.Tensor):
    _need_cuda(w, c)
    w, c = w.contiguous().float(), c.contiguous().float()
    n, d = w.shape
    k = c.shape[0]
    best = torch.empty((n,), dtype=torch.int32, device=w.device)
    score = torch.empty((n,), dtype=torch.float32, device=w.device)
    launch("sd_sim_argmax_f32", w, w.data_ptr(), d, n, d, c.data_ptr(), d, k, best.data_ptr(), score.data_ptr())
    return best, score


def topk_mean_std(x: torch.Tensor, k: int) -> torch.Tensor:
    """[rows, n] f32 -> [rows, 2] = mean and population std of each row's k largest values (k clipped to n).
    Precondition: finite values (a NaN would be selected into the top-k and poison the statistics)."""
    _need_cuda(x)
    x = x.float()
    if x.stride(1) != 1:
        x = x.contiguous()
    rows, n = x.shape
    out = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    launch("sd_topk_mean_std_f32", x, x.data_ptr(), x.stride(0), rows, n, int(k), out.data_ptr())
    return out


def asnorm_scores(query: torch.Tensor, centers: torch.Tensor, cohort: torch.Tensor, topk: int = 200) -> torch.Tensor:
    """`asnorm_scores` [REF diar_diag.py:196-208] on the device: rows scaled by 1 / (norm + 1e-9), the three cosine
    products on the f32 matrix cores (the operator behind the 1x1 convs, T = 1), top-k cohort statistics per row,
    z-normalisation against the query's and the centre's cohort scores, averaged.  f32 [nq, nr].  Precondition: finite inputs."""
    _need_cuda(query, centers, cohort)
    qn, rn, cn = (l2norm_rows(t, eps_add=1e-9) for t in (query, centers, cohort))
    d = qn.shape[1]

    def product(a, b):                                   # a @ b.T with b as the packed "weights" [rows, 1, d_pad]
        wp = pack_weight(b.unsqueeze(2), b.device, torch.float32) if d % 32 else b.reshape(b.shape[0], 1, d).contiguous()
        return conv1d_cl(a, wp, 1, cin=d)

    raw = product(qn, rn)
    k = min(int(topk), cn.shape[0])
    qstat = topk_mean_std(product(qn, cn), k)
    rstat = topk_mean_std(product(rn, cn), k)
    out = torch.empty_like(raw)
    launch("sd_asnorm_combine_f32", raw, raw.data_ptr(), raw.stride(0), raw.shape[0], raw.shape[1], qstat.data_ptr(), rstat.data_ptr(),
           out.data_ptr(), out.stride(0))
    return out


def viterbi(scores: torch.Tensor, alpha: float = 0.995) -> torch.Tensor:
    """`viterbi_hmm` [REF diar_diag.py:231-247] on the device: scores f32 [T, K <= 64] -> int32 path [T]; the two
    transition log-probabilities are formed as the reference forms them (float64 log, rounded to f32).  Precondition: finite
    scores (a NaN candidate is never selected here, np.argmax would return it); K == 1 uses log_move = 0 where the reference
    divides by K - 1 = 0."""
    _need_cuda(scores)
    scores = scores.contiguous().float()
    T, K = scores.shape
    path = torch.empty((T,), dtype=torch.int32, device=scores.device)
    if T == 0:
        return path
    eps = 1e-8
    log_move = float(np.float32(np.log((1 - alpha) / (K - 1) + eps))) if K > 1 else 0.0
    log_stay = float(np.float32(np.log(alpha + eps)))
    nbytes = int(N.load().sd_viterbi_workspace_bytes(T, K))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=scores.device)
    launch("sd_viterbi_f32", scores, scores.data_ptr(), scores.stride(0), T, K, C.c_float(log_stay), C.c_float(log_move), ws.data_ptr(), nbytes,
           path.data_ptr())
    return path


# ----------------------------------------------------------------------------- spectral operator (include/sd_hip_spectral.h)

def affinity_degree(K: torch.Tensor, zero_diag: bool = False) -> torch.Tensor:
    """deg[i] = sum_j max(K[i][j], 0) (without j == i when `zero_diag`) of a square f32 affinity on the GPU -> f32 [N].
    K is read in place (any row stride); bitwise reproducible."""
    _need_cuda(K)
    if K.dtype != torch.float32 or K.dim() != 2 or K.shape[0] != K.shape[1] or K.stride(1) != 1 and K.shape[0] > 1:
        raise ValueError(f"affinity must be a square f32 matrix with contiguous rows, got {tuple(K.shape)} {K.dtype} strides {K.stride()}")
    n = K.shape[0]
    deg = torch.empty((n,), dtype=torch.float32, device=K.device)
    if n == 0:
        return deg
    launch("sd_affinity_degree_f32", K, K.data_ptr(), n, max(K.stride(0), n), int(zero_diag), deg.data_ptr())
    return deg


def rows4(rows: torch.Tensor, what: str = "rows") -> tuple[torch.Tensor, int, int, int]:
    """The rows contract of the entries that read rows (AHC, HDBSCAN, whitening, centres), stated once: a non-empty f32 matrix with
    contiguous rows (`what` names it in the message), a row stride that is a multiple of 4 and a 16-byte aligned base
    -> (view, n, d, row stride).  The view is `rows` itself, read in place (a column slice of a wider matrix is fine); a padded copy
    only when the stride or the alignment demands one."""
    if rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[0] == 0 or rows.shape[1] == 0 or rows.stride(1) != 1 and rows.shape[1] > 1:
        raise ValueError(f"{what} must be a non-empty f32 matrix with contiguous rows, got {tuple(rows.shape)} {rows.dtype} strides {rows.stride()}")
    n, d = rows.shape
    ld = max(rows.stride(0), d) if n > 1 else (d + 3) // 4 * 4              # one row: its stride is never used, any legal value will do
    if ld % 4 or rows.data_ptr() % 16:
        rows = torch.nn.functional.pad(rows, (0, -d % 4))[:, :d] if d % 4 else rows.clone(memory_format=torch.contiguous_format)
        ld = rows.stride(0)
    return rows, n, d, ld


def _workspace(ws, need: int, device) -> torch.Tensor:
    """A workspace of at least `need` bytes: the tensor `ws` if it holds them; otherwise taken from `ws` when it is a `Workspace`, and
    from a fresh one when it is not."""
    if not isinstance(ws, torch.Tensor) or ws.numel() * ws.element_size() < need:
        ws = (ws if isinstance(ws, Workspace) else Workspace(device)).take(need)
    return ws


def affinity_apply(K: torch.Tensor, scale: torch.Tensor, V: torch.Tensor, zero_diag: bool = False,
                   ws: Workspace | torch.Tensor | None = None) -> torch.Tensor:
    """Y = diag(scale) max(K, 0) diag(scale) V on the GPU, the diagonal of K taken as 0 when `zero_diag`.  K f32 [N, N] read in
    place, scale f32 [N], V f32 [N, b] with b in {8, 16, 24, 32} -> f32 [N, b].  `ws`: a `Workspace`, or a uint8 tensor of at least
    sd_affinity_apply_workspace_bytes(N, b), to reuse across calls (allocated when None)."""
    _need_cuda(K, scale, V)
    if K.dtype != torch.float32 or K.dim() != 2 or K.shape[0] != K.shape[1] or K.stride(1) != 1 and K.shape[0] > 1:
        raise ValueError(f"affinity must be a square f32 matrix with contiguous rows, got {tuple(K.shape)} {K.dtype} strides {K.stride()}")
    n = K.shape[0]
    scale = scale.contiguous().float()
    V = V.contiguous().float()
    if scale.shape != (n,) or V.dim() != 2 or V.shape[0] != n:
        raise ValueError(f"scale {tuple(scale.shape)} / V {tuple(V.shape)} do not match the {n} x {n} affinity")
    b = V.shape[1]
    Y = torch.empty((n, b), dtype=torch.float32, device=K.device)
    if n == 0:
        return Y
    ws = _workspace(ws, int(N.load().sd_affinity_apply_workspace_bytes(n, b)), K.device)
    launch("sd_affinity_apply_f32", K, K.data_ptr(), n, max(K.stride(0), n), int(zero_diag), scale.data_ptr(), V.data_ptr(), b, b, Y.data_ptr(), b,
           ws.data_ptr(), ws.numel() * ws.element_size())
    return Y


# ----------------------------------------------------------------------------- average-linkage clustering (include/sd_hip_ahc.h)

def ahc_nearest(sums: torch.Tensor, inv_count: torch.Tensor, ws: Workspace | torch.Tensor | None = None):
    """The nearest other cluster of every cluster under score(i, j) = <sums[i], sums[j]> (inv_count[i] inv_count[j]):
    sums f32 [n, d] under the rows contract (`rows4`), inv_count f32 [n] -> (nn int32 [n], best f32 [n]); exactly symmetric scores,
    lowest index among equal ones, bitwise reproducible.  `ws`: a `Workspace`, or a uint8 tensor of at least
    sd_ahc_nearest_workspace_bytes(n, d), to reuse across calls (allocated when None)."""
    _need_cuda(sums, inv_count)
    sums, n, d, ld = rows4(sums, "cluster sums")
    inv_count = inv_count.contiguous().float()
    if inv_count.shape != (n,):
        raise ValueError(f"inv_count {tuple(inv_count.shape)} does not match the {n} cluster sums")
    nn = torch.empty((n,), dtype=torch.int32, device=sums.device)
    best = torch.empty((n,), dtype=torch.float32, device=sums.device)
    ws = _workspace(ws, int(N.load().sd_ahc_nearest_workspace_bytes(n, d)), sums.device)
    launch("sd_ahc_nearest_f32", sums, sums.data_ptr(), ld, n, d, inv_count.data_ptr(), nn.data_ptr(), best.data_ptr(),
           ws.data_ptr(), ws.numel() * ws.element_size())
    return nn, best


def ahc_nearest_grouped(sums: torch.Tensor, inv_count: torch.Tensor, group: torch.Tensor, max_group: int,
                        ws: Workspace | torch.Tensor | None = None):
    """`ahc_nearest` over the clusters of many recordings at once: group int32 [n], non-decreasing, names the recording of every
    cluster, and only a cluster of the same recording is a neighbour; `max_group` bounds the clusters of any one recording
    -> (nn int32 [n], indices into all n rows, -1 for a cluster alone in its recording; best f32 [n]; bad int32 [1], still on the
    device: non-zero when `group` decreases somewhere or a group exceeds `max_group`, and nn / best mean nothing then).  The scores of
    a recording are bit for bit those of `ahc_nearest` on its rows alone.  `ws`: a `Workspace`, or a uint8 tensor of at least
    sd_ahc_nearest_grouped_workspace_bytes(n, d, max_group), to reuse across calls (allocated when None)."""
    _need_cuda(sums, inv_count, group)
    sums, n, d, ld = rows4(sums, "cluster sums")
    inv_count = inv_count.contiguous().float()
    if inv_count.shape != (n,):
        raise ValueError(f"inv_count {tuple(inv_count.shape)} does not match the {n} cluster sums")
    if group.dtype != torch.int32 or group.shape != (n,) or not group.is_contiguous():
        raise ValueError(f"group must be a contiguous {torch.int32} vector of {n} entries, got {tuple(group.shape)} {group.dtype}")
    max_group = int(max_group)
    nn = torch.empty((n,), dtype=torch.int32, device=sums.device)
    best = torch.empty((n,), dtype=torch.float32, device=sums.device)
    bad = torch.empty((1,), dtype=torch.int32, device=sums.device)
    ws = _workspace(ws, int(N.load().sd_ahc_nearest_grouped_workspace_bytes(n, d, max_group)), sums.device)
    launch("sd_ahc_nearest_grouped_f32", sums, sums.data_ptr(), ld, n, d, inv_count.data_ptr(), group.data_ptr(), max_group, nn.data_ptr(),
           best.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
    return nn, best, bad


def ahc_merge(sums: torch.Tensor, count: torch.Tensor, inv_count: torch.Tensor, nn: torch.Tensor, best: torch.Tensor, cos_thr: float):
    """One round of merges IN PLACE: every reciprocal pair i < j (nn[i] == j, nn[j] == i) with best[i] > cos_thr adds row j of `sums`
    and its count into row i and refreshes inv_count[i] -> (target int32 [n]: i for the upper row of a pair, the row itself otherwise;
    n_merged int32 [1], still on the device)."""
    _need_cuda(sums, count, inv_count, nn, best)
    view, n, d, ld = rows4(sums, "cluster sums")
    if view is not sums:
        raise ValueError(f"cluster sums are merged in place: a row stride that is a multiple of 4 and a 16-byte aligned base, got strides {sums.stride()}")
    for name, t, dt in (("count", count, torch.float32), ("inv_count", inv_count, torch.float32), ("nn", nn, torch.int32),
                        ("best", best, torch.float32)):
        if t.dtype != dt or t.shape != (n,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} vector of {n} entries, got {tuple(t.shape)} {t.dtype}")
    target = torch.empty((n,), dtype=torch.int32, device=sums.device)
    n_merged = torch.empty((1,), dtype=torch.int32, device=sums.device)
    launch("sd_ahc_merge_f32", sums, sums.data_ptr(), ld, n, d, count.data_ptr(), inv_count.data_ptr(), nn.data_ptr(), best.data_ptr(),
           C.c_float(cos_thr), target.data_ptr(), n_merged.data_ptr())
    return target, n_merged


# ----------------------------------------------------------------------------- the bounded cut of the AHC merge log (include/sd_hip_cut.h)

def ahc_cut_grouped(lo: torch.Tensor, hi: torch.Tensor, key: torch.Tensor, first_merge: torch.Tensor, first_row: torch.Tensor,
                    cos_thr: float, min_clusters: torch.Tensor, max_clusters: torch.Tensor, ws: Workspace | torch.Tensor | None = None):
    """The labels of many recordings at a bounded cluster count from their merge logs, in one launch: lo, hi int32 [M] (the lowest
    rows of the kept and the absorbed cluster, counted from the recording's first row), key f32 [M] (finite), first_merge and first_row
    int32 [G + 1] (non-decreasing, 0 first, M and the number of rows last), min_clusters and max_clusters int32 [G]
    -> (labels int32 [rows], the rows of recording g from first_row[g] on, numbered by first appearance; clusters int32 [G]; bad
    int32 [G]; all still on the device).  Per recording the m = max(0, min(max(c, n - max), n - min)) first merges in the order (key
    descending, position ascending) are applied, c the merges with key > cos_thr; bad is non-zero, and the labels all -1, where the
    log of a recording is broken (include/sd_hip_cut.h has the list).  `ws`: a `Workspace`, or a uint8 tensor of at least
    sd_ahc_cut_workspace_bytes(rows, G), to reuse across calls (allocated when None).  The number of rows is read from
    first_row[G]: one synchronisation, which the caller's read of `bad` would make anyway."""
    _need_cuda(lo, hi, key, first_merge, first_row, min_clusters, max_clusters)
    M, G = key.numel(), first_row.numel() - 1
    for name, t, dt, n in (("lo", lo, torch.int32, M), ("hi", hi, torch.int32, M), ("key", key, torch.float32, M),
                           ("first_merge", first_merge, torch.int32, G + 1), ("first_row", first_row, torch.int32, G + 1),
                           ("min_clusters", min_clusters, torch.int32, G), ("max_clusters", max_clusters, torch.int32, G)):
        if t.dtype != dt or t.shape != (n,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} vector of {n} entries, got {tuple(t.shape)} {t.dtype}")
    if G < 1:
        raise ValueError("first_row must name at least one recording")
    rows = int(first_row[-1])                       # the one number the output's size hangs on
    if rows < 0:
        raise ValueError(f"first_row ends at {rows}")
    dev = key.device
    labels = torch.empty((rows,), dtype=torch.int32, device=dev)
    clusters = torch.empty((G,), dtype=torch.int32, device=dev)
    bad = torch.empty((G,), dtype=torch.int32, device=dev)
    ws = _workspace(ws, int(N.load().sd_ahc_cut_workspace_bytes(rows, G)), dev)
    launch("sd_ahc_cut_grouped", first_row, _ptr(lo) or None, _ptr(hi) or None, _ptr(key) or None, first_merge.data_ptr(), first_row.data_ptr(), G, M,
           rows, C.c_float(cos_thr), min_clusters.data_ptr(), max_clusters.data_ptr(), labels.data_ptr() or None, clusters.data_ptr(), bad.data_ptr(),
           ws.data_ptr(), ws.numel() * ws.element_size())
    return labels, clusters, bad


# ----------------------------------------------------------------------------- k-means (include/sd_hip_kmeans.h)

def kmeans_grouped(rows: torch.Tensor, first_row: torch.Tensor, k: torch.Tensor, first: torch.Tensor, u: torch.Tensor, n_init: int,
                   max_iter: int, tol: float, max_k: int = 32, max_rows: int | None = None, ws: Workspace | torch.Tensor | None = None):
    """scikit-learn's `k_means(rows_g, k[g], n_init=n_init, max_iter=max_iter, tol=tol)` labels for many recordings in two launches
    (the restarts, then the selection among them), the random numbers supplied: rows f64 [n, dim <= 32] read in place (contiguous
    columns, any row stride), first_row int32 [G + 1] (non-decreasing, 0 first, n last), k int32 [G] (2 <= k <= max_k <= 32, k below
    the recording's rows), first int32 [G, n_init] (the row of every restart's first centre), u f64 [G, n_init, 31, 5] (the uniform
    numbers of the seeding; `kmeans_gpu.kmeans_draws` makes both) -> (labels int32 [n], chosen int32 [G], inertia f64 [G], iters
    int32 [G], flags int32 [G]; all still on the device).  `flags` is non-zero, and the recording's labels all -1, where a cluster ran
    empty, a row is not finite or an argument of the recording is out of range (include/sd_hip_kmeans.h has the values).  `max_rows`:
    a bound on the rows of one recording, up to which they are kept in LDS (default: all n).  `ws`: a `Workspace`, or a uint8 tensor
    of at least sd_kmeans_grouped_workspace_bytes(n, G, n_init), to reuse across calls (allocated when None)."""
    _need_cuda(rows, first_row, k, first, u)
    if rows.dtype != torch.float64 or rows.dim() != 2 or rows.shape[1] == 0 or rows.stride(1) != 1 and rows.shape[1] > 1:
        raise ValueError(f"rows must be an f64 matrix with contiguous columns, got {tuple(rows.shape)} {rows.dtype} strides {rows.stride()}")
    n, dim = rows.shape
    G, n_init = k.numel(), int(n_init)
    ld = max(rows.stride(0), dim) if n > 1 else dim
    for name, t, dt, shape in (("first_row", first_row, torch.int32, (G + 1,)), ("k", k, torch.int32, (G,)),
                               ("first", first, torch.int32, (G, n_init)), ("u", u, torch.float64, (G, n_init, 31, 5))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} tensor of shape {shape}, got {tuple(t.shape)} {t.dtype}")
    dev = rows.device
    labels = torch.empty((n,), dtype=torch.int32, device=dev)
    chosen, iters, flags = (torch.empty((G,), dtype=torch.int32, device=dev) for _ in range(3))
    inertia = torch.empty((G,), dtype=torch.float64, device=dev)
    ws = _workspace(ws, int(N.load().sd_kmeans_grouped_workspace_bytes(n, G, n_init)), dev)
    launch("sd_kmeans_grouped_f64", rows, rows.data_ptr() or None, ld, n, dim, first_row.data_ptr(), G, k.data_ptr(), n_init, int(max_iter),
           C.c_double(tol), int(max_k), int(n if max_rows is None else max_rows) or 1, first.data_ptr(), u.data_ptr(), labels.data_ptr() or None,
           chosen.data_ptr(), inertia.data_ptr(), iters.data_ptr(), flags.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
    return labels, chosen, inertia, iters, flags


# ----------------------------------------------------------------------------- voice activity (include/sd_hip_vad.h)

def _table(name: str, t: torch.Tensor, dt, n: int) -> None:
    if t.dtype != dt or tuple(t.shape) != (n,) or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dt} tensor of shape ({n},), got {tuple(t.shape)} {t.dtype}")


def vad_energy_grouped(signal: torch.Tensor, first_sample: torch.Tensor, n_samples: torch.Tensor, first_frame: torch.Tensor, n_frames: int,
                       win: int, hop: int, threshold_db: float, slope: float):
    """`vad.EnergyScorer(threshold_db, slope)` over `vad.frame_audio` for many recordings in one launch: signal f32 [n] (1-d,
    contiguous), recording g its samples [first_sample[g], first_sample[g] + n_samples[g]) (int64 [G], int32 [G]), frames of `win`
    samples every `hop`, first_frame int32 [G + 1] the prefix sums of the frame counts 1 + (n_samples - win) // hop, n_frames their
    total -> (probs f32 [n_frames], bad int32 [G]; both still on the device).  `bad` is non-zero, and the recording's probabilities
    NaN, where a recording is shorter than a frame, leaves the signal or disagrees with first_frame (include/sd_hip_vad.h)."""
    _need_cuda(signal, first_sample, n_samples, first_frame)
    if signal.dtype != torch.float32 or signal.dim() != 1 or not signal.is_contiguous():
        raise ValueError(f"signal must be a contiguous 1-d f32 tensor, got {tuple(signal.shape)} {signal.dtype}")
    G = n_samples.numel()
    _table("first_sample", first_sample, torch.int64, G)
    _table("n_samples", n_samples, torch.int32, G)
    _table("first_frame", first_frame, torch.int32, G + 1)
    probs = torch.empty((int(n_frames),), dtype=torch.float32, device=signal.device)
    bad = torch.empty((G,), dtype=torch.int32, device=signal.device)
    launch("sd_vad_energy_grouped_f32", signal, signal.data_ptr() or None, signal.numel(), first_sample.data_ptr(), n_samples.data_ptr(), G,
           int(win), int(hop), float(threshold_db), float(slope), first_frame.data_ptr(), int(n_frames), probs.data_ptr() or None, bad.data_ptr())
    return probs, bad


def vad_segments_grouped(probs: torch.Tensor, first_frame: torch.Tensor, first_seg: torch.Tensor, seg_cap: int, on: float, off: float,
                         open_len: int, close_len: int, min_run: int, max_gap: int, want_mask: bool = False,
                         ws: Workspace | torch.Tensor | None = None):
    """Frame probabilities to speech runs for many recordings in one launch (`vad.hysteresis_binarize`, `vad.morph_open_close` with
    lines of open_len and close_len frames, and the run rules of `vad.mask_to_segments` before its padding): probs f32 [n_frames],
    first_frame int32 [G + 1] (non-decreasing, 0 first, n_frames last), first_seg int32 [G + 1] likewise with seg_cap last, every
    recording's share at least (its frames + 1) // 2 -> (n_segs int32 [G], seg_start int32 [seg_cap], seg_end int32 [seg_cap],
    mask uint8 [n_frames] or None, bad int32 [G]; all still on the device).  `ws`: a `Workspace`, or a uint8 tensor of at least
    sd_vad_segments_workspace_bytes(seg_cap, G), to reuse across calls (allocated when None)."""
    _need_cuda(probs, first_frame, first_seg)
    if probs.dtype != torch.float32 or probs.dim() != 1 or not probs.is_contiguous():
        raise ValueError(f"probs must be a contiguous 1-d f32 tensor, got {tuple(probs.shape)} {probs.dtype}")
    G, n_frames, seg_cap = first_frame.numel() - 1, probs.numel(), int(seg_cap)
    _table("first_frame", first_frame, torch.int32, G + 1)
    _table("first_seg", first_seg, torch.int32, G + 1)
    dev = probs.device
    n_segs, bad = (torch.empty((G,), dtype=torch.int32, device=dev) for _ in range(2))
    seg_start, seg_end = (torch.empty((seg_cap,), dtype=torch.int32, device=dev) for _ in range(2))
    mask = torch.empty((n_frames,), dtype=torch.uint8, device=dev) if want_mask else None
    ws = _workspace(ws, int(N.load().sd_vad_segments_workspace_bytes(seg_cap, G)), dev)
    launch("sd_vad_segments_grouped", first_frame, probs.data_ptr() or None, first_frame.data_ptr(), G, n_frames, float(on), float(off),
           int(open_len), int(close_len), int(min_run), int(max_gap), first_seg.data_ptr(), seg_cap, n_segs.data_ptr(),
           seg_start.data_ptr() or None, seg_end.data_ptr() or None, (_ptr(mask) or None) if want_mask else None, bad.data_ptr(),
           ws.data_ptr(), ws.numel() * ws.element_size())
    return n_segs, seg_start, seg_end, mask, bad


# ----------------------------------------------------------------------------- speaker-change detection (include/sd_hip_scd.h)

def scd_split_grouped(rows: torch.Tensor, first_row: torch.Tensor, seg_start: torch.Tensor, seg_end: torch.Tensor, first_piece: torch.Tensor,
                      piece_cap: int, hop_ms: float, thr: float, min_speech_s: float, eps: float = 1e-8, want_sims: bool = False,
                      want_mask: bool = False, ws: Workspace | torch.Tensor | None = None):
    """Pass 2 of `anti_stick_diarize.scd_split_segments` for many segments in one launch: rows f32 [n_rows, dim] (unit stride inside a
    row), segment g its rows [first_row[g], first_row[g + 1]) (int32 [G + 1], non-decreasing, 0 first, n_rows last) between
    seg_start[g] and seg_end[g] seconds (f64 [G]), first_piece int32 [G + 1] likewise with piece_cap last, every segment's share at
    least max(1, its rows // 2) -> (n_peaks int32 [G], n_pieces int32 [G], piece_start f64 [piece_cap], piece_end f64 [piece_cap],
    sims f32 [n_rows] or None, peak_mask uint8 [n_rows] or None, bad int32 [G]; all still on the device).  `ws`: a `Workspace`, or a
    uint8 tensor of at least sd_scd_split_workspace_bytes(n_rows, G), to reuse across calls (allocated when None)."""
    _need_cuda(rows, first_row, seg_start, seg_end, first_piece)
    if rows.dtype != torch.float32 or rows.dim() != 2 or (rows.shape[1] > 1 and rows.stride(1) != 1) or (rows.shape[0] > 1 and rows.stride(0) < rows.shape[1]):
        raise ValueError(f"rows must be a 2-d f32 tensor with unit stride inside a row, got {tuple(rows.shape)} {rows.dtype} strides {rows.stride()}")
    n_rows, dim = int(rows.shape[0]), int(rows.shape[1])
    ld = int(rows.stride(0)) if n_rows > 1 else dim
    G, piece_cap = first_row.numel() - 1, int(piece_cap)
    _table("first_row", first_row, torch.int32, G + 1)
    _table("first_piece", first_piece, torch.int32, G + 1)
    _table("seg_start", seg_start, torch.float64, G)
    _table("seg_end", seg_end, torch.float64, G)
    dev = rows.device
    n_peaks, n_pieces, bad = (torch.empty((G,), dtype=torch.int32, device=dev) for _ in range(3))
    piece_start, piece_end = (torch.empty((piece_cap,), dtype=torch.float64, device=dev) for _ in range(2))
    sims = torch.empty((n_rows,), dtype=torch.float32, device=dev) if want_sims else None
    mask = torch.empty((n_rows,), dtype=torch.uint8, device=dev) if want_mask else None
    ws = _workspace(ws, int(N.load().sd_scd_split_workspace_bytes(n_rows, G)), dev)
    launch("sd_scd_split_grouped_f32", rows, rows.data_ptr() or None, ld, dim, n_rows, first_row.data_ptr(), G, seg_start.data_ptr(),
           seg_end.data_ptr(), C.c_double(hop_ms), C.c_double(thr), C.c_double(min_speech_s), C.c_float(eps), first_piece.data_ptr(), piece_cap,
           n_peaks.data_ptr(), n_pieces.data_ptr(), piece_start.data_ptr() or None, piece_end.data_ptr() or None, _ptr(sims) or None,
           _ptr(mask) or None, bad.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
    return n_peaks, n_pieces, piece_start, piece_end, sims, mask, bad


# ----------------------------------------------------------------------------- speaker turns (include/sd_hip_turns.h)

def turns_grouped(first_window: torch.Tensor, first_region: torch.Tensor, region_first_window: torch.Tensor, centre: torch.Tensor,
                  region_start: torch.Tensor, n_frames: torch.Tensor, frame_s: float, labels: torch.Tensor,
                  ws: Workspace | torch.Tensor | None = None):
    """`cluster.relabel_by_first_appearance` and the runs of `diarization_baseline.labels_to_turns` for many recordings in one launch:
    recording g its windows [first_window[g], first_window[g + 1]) and its regions [first_region[g], first_region[g + 1]) (int32
    [G + 1], non-decreasing, 0 first), region r its windows [region_first_window[r], region_first_window[r + 1]) (int32 [R + 1]), the
    window centres f64 [W] in seconds, region_start f64 [R], n_frames int32 [R], labels int32 [W] -> (new_labels int32 [W], n_runs
    int32 [G], run_region, run_first, run_end, run_label int32 [W] with a recording's runs from first_window[g] on, bad int32 [G]; all
    still on the device).  `bad` is non-zero, and the recording has no runs, where a label is not below the recording's window count
    or a table, the centres or the frame counts break their promise (include/sd_hip_turns.h).  `ws`: a `Workspace`, or a uint8 tensor
    of at least sd_turns_workspace_bytes(W, G), to reuse across calls (allocated when None)."""
    _need_cuda(first_window, first_region, region_first_window, centre, region_start, n_frames, labels)
    G, R, W = first_window.numel() - 1, region_first_window.numel() - 1, labels.numel()
    _table("first_window", first_window, torch.int32, G + 1)
    _table("first_region", first_region, torch.int32, G + 1)
    _table("region_first_window", region_first_window, torch.int32, R + 1)
    _table("centre", centre, torch.float64, W)
    _table("region_start", region_start, torch.float64, R)
    _table("n_frames", n_frames, torch.int32, R)
    _table("labels", labels, torch.int32, W)
    dev = labels.device
    new_labels, run_region, run_first, run_end, run_label = (torch.empty((W,), dtype=torch.int32, device=dev) for _ in range(5))
    n_runs, bad = (torch.empty((G,), dtype=torch.int32, device=dev) for _ in range(2))
    ws = _workspace(ws, int(N.load().sd_turns_workspace_bytes(W, G)), dev)
    launch("sd_turns_grouped", labels, first_window.data_ptr(), first_region.data_ptr(), G, region_first_window.data_ptr(), R,
           centre.data_ptr() or None, W, region_start.data_ptr() or None, n_frames.data_ptr() or None, C.c_double(frame_s),
           labels.data_ptr() or None, new_labels.data_ptr() or None, n_runs.data_ptr(), run_region.data_ptr() or None,
           run_first.data_ptr() or None, run_end.data_ptr() or None, run_label.data_ptr() or None, bad.data_ptr(), ws.data_ptr(),
           ws.numel() * ws.element_size())
    return new_labels, n_runs, run_region, run_first, run_end, run_label, bad


# ----------------------------------------------------------------------------- density clustering (include/sd_hip_hdbscan.h)

def hdb_core(rows: torch.Tensor, k: int, ws: Workspace | torch.Tensor | None = None) -> torch.Tensor:
    """core[i] = the k-th largest <rows[i], rows[j]> over j != i, duplicates counted (1 <= k <= min(16, n - 1)): rows f32 [n, d] under
    the rows contract (`rows4`) -> f32 [n].  The products are those of `hdb_outgoing`, bit for bit.  `ws`: a `Workspace`, or a uint8
    tensor of at least sd_hdb_core_workspace_bytes(n, d, k), to reuse across calls (allocated when None)."""
    _need_cuda(rows)
    rows, n, d, ld = rows4(rows)
    core = torch.empty((n,), dtype=torch.float32, device=rows.device)
    ws = _workspace(ws, int(N.load().sd_hdb_core_workspace_bytes(n, d, int(k))), rows.device)
    launch("sd_hdb_core_f32", rows, rows.data_ptr(), ld, n, d, int(k), core.data_ptr(),
           ws.data_ptr(), ws.numel() * ws.element_size())
    return core


def hdb_outgoing(rows: torch.Tensor, core: torch.Tensor, comp: torch.Tensor, ws: Workspace | torch.Tensor | None = None):
    """The heaviest edge that leaves the component of every row under w(i, j) = min(core[i], core[j], <rows[i], rows[j]>):
    rows f32 [n, d] as for `hdb_core`, core f32 [n] (+inf allowed), comp int32 [n] -> (nn int32 [n], best f32 [n]); nn = -1 and
    best = -inf for a row whose component is everything.  Exactly symmetric w, lowest index among equal ones, bitwise reproducible.
    `ws`: a `Workspace`, or a uint8 tensor of at least sd_hdb_outgoing_workspace_bytes(n, d), to reuse across calls (allocated when
    None)."""
    _need_cuda(rows, core, comp)
    rows, n, d, ld = rows4(rows)
    for name, t, dt in (("core", core, torch.float32), ("comp", comp, torch.int32)):
        if t.dtype != dt or t.shape != (n,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} vector of {n} entries, got {tuple(t.shape)} {t.dtype}")
    nn = torch.empty((n,), dtype=torch.int32, device=rows.device)
    best = torch.empty((n,), dtype=torch.float32, device=rows.device)
    ws = _workspace(ws, int(N.load().sd_hdb_outgoing_workspace_bytes(n, d)), rows.device)
    launch("sd_hdb_outgoing_f32", rows, rows.data_ptr(), ld, n, d, core.data_ptr(), comp.data_ptr(), nn.data_ptr(), best.data_ptr(),
           ws.data_ptr(), ws.numel() * ws.element_size())
    return nn, best


def _group_vector(group: torch.Tensor, n: int) -> None:
    if group.dtype != torch.int32 or group.shape != (n,) or not group.is_contiguous():
        raise ValueError(f"group must be a contiguous {torch.int32} vector of {n} entries, got {tuple(group.shape)} {group.dtype}")


def hdb_core_grouped(rows: torch.Tensor, k: int, group: torch.Tensor, max_group: int, ws: Workspace | torch.Tensor | None = None):
    """`hdb_core` over the rows of many recordings at once: group int32 [n], non-decreasing, names the recording of every row, and only
    a row of the same recording counts; `max_group` bounds the rows of any one recording -> (core f32 [n], -inf for a row with fewer
    than k others in its recording; bad int32 [1], still on the device: non-zero when `group` decreases somewhere or a group exceeds
    `max_group`, and core means nothing then).  1 <= k <= 16.  A recording's values are bit for bit those of `hdb_core` on its rows
    alone.  `ws`: a `Workspace`, or a uint8 tensor of at least sd_hdb_core_grouped_workspace_bytes(n, d, k, max_group)."""
    _need_cuda(rows, group)
    rows, n, d, ld = rows4(rows)
    _group_vector(group, n)
    k, max_group = int(k), int(max_group)
    core = torch.empty((n,), dtype=torch.float32, device=rows.device)
    bad = torch.empty((1,), dtype=torch.int32, device=rows.device)
    ws = _workspace(ws, int(N.load().sd_hdb_core_grouped_workspace_bytes(n, d, k, max_group)), rows.device)
    launch("sd_hdb_core_grouped_f32", rows, rows.data_ptr(), ld, n, d, k, group.data_ptr(), max_group, core.data_ptr(), bad.data_ptr(),
           ws.data_ptr(), ws.numel() * ws.element_size())
    return core, bad


def hdb_outgoing_grouped(rows: torch.Tensor, core: torch.Tensor, comp: torch.Tensor, group: torch.Tensor, max_group: int,
                         ws: Workspace | torch.Tensor | None = None):
    """`hdb_outgoing` over the rows of many recordings at once (group, max_group and bad as for `hdb_core_grouped`): the heaviest edge
    into another component of the row's OWN recording -> (nn int32 [n], indices into all n rows, -1 for a row whose component is its
    whole recording; best f32 [n]; bad int32 [1], still on the device).  A recording's weights are bit for bit those of `hdb_outgoing`
    on its rows alone.  `ws`: a `Workspace`, or a uint8 tensor of at least sd_hdb_outgoing_grouped_workspace_bytes(n, d, max_group)."""
    _need_cuda(rows, core, comp, group)
    rows, n, d, ld = rows4(rows)
    for name, t, dt in (("core", core, torch.float32), ("comp", comp, torch.int32)):
        if t.dtype != dt or t.shape != (n,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} vector of {n} entries, got {tuple(t.shape)} {t.dtype}")
    _group_vector(group, n)
    max_group = int(max_group)
    nn = torch.empty((n,), dtype=torch.int32, device=rows.device)
    best = torch.empty((n,), dtype=torch.float32, device=rows.device)
    bad = torch.empty((1,), dtype=torch.int32, device=rows.device)
    ws = _workspace(ws, int(N.load().sd_hdb_outgoing_grouped_workspace_bytes(n, d, max_group)), rows.device)
    launch("sd_hdb_outgoing_grouped_f32", rows, rows.data_ptr(), ld, n, d, core.data_ptr(), comp.data_ptr(), group.data_ptr(), max_group,
           nn.data_ptr(), best.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
    return nn, best, bad


# ----------------------------------------------------------------------------- from the tree's edges to the labels (include/sd_hip_tree.h)

def tree_labels_grouped(lo: torch.Tensor, hi: torch.Tensor, dist: torch.Tensor, first_edge: torch.Tensor, max_edges: int,
                        min_cluster_size: int, allow_single_cluster: bool, ws: Workspace | torch.Tensor | None = None):
    """HDBSCAN's labels from the spanning trees of many recordings in one launch: lo, hi int32 [E] (rows counted from the recording's
    first), dist f64 [E] (finite, >= 0), first_edge int32 [G + 1] (non-decreasing, 0 first, E last; recording g owns the edges
    [first_edge[g], first_edge[g + 1]), at least one), `max_edges` a bound on the edges of any one recording -> (labels int32 [E + G],
    the rows of recording g from first_edge[g] + g on; bad int32 [G], still on the device: non-zero where a recording's edges are no
    spanning tree of its rows or a distance is negative or not finite, and that recording's labels are all -1).  Per recording exactly
    scikit-learn 1.7.2's `tree_to_labels(make_single_linkage(mst[argsort(dist, kind="stable")]), min_cluster_size, "eom",
    allow_single_cluster, 0.0, None)[0]`.  `ws`: a `Workspace`, or a uint8 tensor of at least
    sd_tree_labels_workspace_bytes(E, G, max_edges), to reuse across calls (allocated when None)."""
    _need_cuda(lo, hi, dist, first_edge)
    E, G = dist.numel(), first_edge.numel() - 1
    for name, t, dt, n in (("lo", lo, torch.int32, E), ("hi", hi, torch.int32, E), ("dist", dist, torch.float64, E),
                           ("first_edge", first_edge, torch.int32, G + 1)):
        if t.dtype != dt or t.shape != (n,) or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} vector of {n} entries, got {tuple(t.shape)} {t.dtype}")
    max_edges = int(max_edges)
    labels = torch.empty((E + max(G, 0),), dtype=torch.int32, device=dist.device)
    bad = torch.empty((max(G, 0),), dtype=torch.int32, device=dist.device)
    ws = _workspace(ws, int(N.load().sd_tree_labels_workspace_bytes(E, G, max_edges)), dist.device)
    launch("sd_tree_labels_grouped", dist, lo.data_ptr(), hi.data_ptr(), dist.data_ptr(), first_edge.data_ptr(), G, E, max_edges,
           int(min_cluster_size), int(bool(allow_single_cluster)), labels.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
    return labels, bad


# ----------------------------------------------------------------------------- f64 whitening and cluster centres (include/sd_hip_diag.h)

def whiten_stats(rows: torch.Tensor, ws: Workspace | torch.Tensor | None = None):
    """Column means and the centred Gram matrix of rows f32 [n >= 2, d <= 256] in f64 on the f64 matrix cores, two passes as np.cov:
    -> (mean f64 [d], gram f64 [d, d] = sum_i (x_i - mean)^T (x_i - mean), exactly symmetric; divide by n - 1 for the covariance).
    Rows under the rows contract (`rows4`); bitwise reproducible, the summation order depends on (n, d) alone.  `ws`: a `Workspace`,
    or a uint8 tensor of at least sd_whiten_stats_workspace_bytes(n, d), to reuse across calls (allocated when None)."""
    _need_cuda(rows)
    rows, n, d, ld = rows4(rows)
    mean = torch.empty((d,), dtype=torch.float64, device=rows.device)
    gram = torch.empty((d, d), dtype=torch.float64, device=rows.device)
    ws = _workspace(ws, int(N.load().sd_whiten_stats_workspace_bytes(n, d)), rows.device)
    launch("sd_whiten_stats_f64", rows, rows.data_ptr(), ld, n, d, mean.data_ptr(), gram.data_ptr(), d,
           ws.data_ptr(), ws.numel() * ws.element_size())
    return mean, gram


def whiten_apply(rows: torch.Tensor, mean: torch.Tensor, W: torch.Tensor, eps_add: float = 1e-9) -> torch.Tensor:
    """out[i] = f32(v / (||v|| + eps_add)), v = (rows[i] - mean) @ W in f64 on the f64 matrix cores: rows f32 [n, d <= 256] read in
    place, mean f64 [d], W f64 [d, d] (symmetry is not assumed) -> f32 [n, d]; one rounding to f32."""
    _need_cuda(rows, mean, W)
    rows, n, d, ld = rows4(rows)
    mean = mean.contiguous()
    W = W.contiguous()
    if mean.dtype != torch.float64 or mean.shape != (d,) or W.dtype != torch.float64 or W.shape != (d, d):
        raise ValueError(f"mean {tuple(mean.shape)} {mean.dtype} / W {tuple(W.shape)} {W.dtype} must be f64 [{d}] and f64 [{d}, {d}]")
    out = torch.empty((n, d), dtype=torch.float32, device=rows.device)
    launch("sd_whiten_apply_f64", rows, rows.data_ptr(), ld, n, d, mean.data_ptr(), W.data_ptr(), d, C.c_double(eps_add), out.data_ptr(), d)
    return out


def label_centroids(rows: torch.Tensor, labels: torch.Tensor, k: int, eps_add: float = 1e-9):
    """The unit mean of every label's rows: rows f32 [n, d <= 256] read in place, labels int32 [n], 1 <= k <= 1024 ->
    (centres f32 [k, d], count int32 [k]).  The mean is accumulated in f64 in ascending row order and divided by (its norm + eps_add);
    a label outside [0, k) is skipped, a label without rows gives a zero row and count 0."""
    _need_cuda(rows, labels)
    rows, n, d, ld = rows4(rows)
    if labels.dtype != torch.int32 or labels.shape != (n,) or not labels.is_contiguous():
        raise ValueError(f"labels must be a contiguous int32 vector of {n} entries, got {tuple(labels.shape)} {labels.dtype}")
    k = int(k)
    out = torch.empty((max(k, 0), d), dtype=torch.float32, device=rows.device)
    count = torch.empty((max(k, 0),), dtype=torch.int32, device=rows.device)
    launch("sd_label_centroids_f32", rows, rows.data_ptr(), ld, n, d, labels.data_ptr(), k, C.c_double(eps_add), out.data_ptr(), d, count.data_ptr())
    return out, count


def rows_product(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a @ b.T of f32 rows a [n, d], b [k, d] -> f32 [n, k] on the f32 matrix cores (exact f32 products): the operator behind the
    1x1 convs at T = 1 with b as the packed weights, as the three products of `asnorm_scores`."""
    _need_cuda(a, b)
    a, b = a.contiguous().float(), b.contiguous().float()
    d = a.shape[1]
    wp = pack_weight(b.unsqueeze(2), b.device, torch.float32) if d % 32 else b.reshape(b.shape[0], 1, d).contiguous()
    return conv1d_cl(a, wp, 1, cin=d)
