"""Device-resident embedding engine: waveform [B, n] on the GPU -> 192-d embeddings on the GPU.

This is the host side of the hot path: it owns the packed weights, the fbank plan
and one workspace in HBM, and issues `sd_fbank_f32` + `sd_ecapa_forward_f32` on the
current torch stream.  PyTorch is used for device memory and streams only; all
arithmetic is in libsd_hip.so.

The reference re-creates its feature transform and crosses host<->device three times
per batch [REF speech_encode.py:17-38,76-77]; here tables and weights are uploaded
once and a batch costs one H2D (waveforms) and one D2H (embeddings) at the API edge.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np
import torch

from . import _native as N
from . import ops
from .features import HOP, FbankPlan
from .synth import EcapaConfig, config_from_state_dict

BN_EPS = 1e-5  # torch.nn.BatchNorm1d default, as used by speechbrain's BatchNorm1d
K_ALIGN = 32   # K step of the conv/GEMM kernel


def min_frames(cfg: EcapaConfig) -> int:
    """The shortest segment, in frames, the network takes: every "same" conv pads with reflection, which needs pad < T, and the
    largest pad is max dil * (k - 1) / 2 over the convs (the k = 1 layers pad nothing).  5 for the spkrec geometry (k = 3, dil = 4)."""
    return 1 + max(d * (k - 1) // 2 for k, d in zip(cfg.kernel_sizes, cfg.dilations))


def min_samples(cfg: EcapaConfig) -> int:
    """The shortest segment in samples: T = 1 + n // 160 frames, so (min_frames - 1) * 160.  640 for the spkrec geometry."""
    return (min_frames(cfg) - 1) * HOP


SPAN_BUDGET_FRAMES = 201   # default frame budget of a packed micro-batch: this many frames (one 2 s segment) per max_batch


def span_frame_offsets(lengths) -> np.ndarray:
    """Packed spans (include/sd_hip.h): span s of n_s samples has T_s = 1 + n_s // 160 frames, stored back to back in span order.
    -> frame_start int32 [B + 1]: frame_start[s] = sum of T_r over r < s, frame_start[B] = M, the rows of the pack."""
    n = np.asarray(lengths, dtype=np.int64).reshape(-1)
    out = np.zeros(n.size + 1, np.int64)
    np.cumsum(1 + n // HOP, out=out[1:])
    if out[-1] >= 2 ** 31:
        raise ValueError(f"packed spans: {int(out[-1])} frames do not fit one launch (at most 2^31 - 1)")
    return out.astype(np.int32)


def plan_span_batches(frames, budget: int) -> list:
    """Micro-batches of packed spans: consecutive runs [lo, hi) in span order whose frames add up to at most `budget`; a span is never
    split, and one longer than the budget goes alone."""
    out, lo, acc = [], 0, 0
    for i, f in enumerate(int(x) for x in frames):
        if i > lo and acc + f > budget:
            out.append((lo, i))
            lo, acc = i, 0
        acc += f
    if len(frames) > lo:
        out.append((lo, len(frames)))
    return out


def check_spans(starts, lengths, n_total: int, min_samples_: int, min_frames_: int):
    """Host validation of packed spans, before anything is launched -> (starts int64 [B], lengths int64 [B]).  Every span must lie
    inside the signal (no zero fill: `embed_windows` does that) and have at least `min_samples_` samples (the network's floor)."""
    def ints(v, what):
        a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
        if a.ndim != 1:
            raise ValueError(f"{what} must be a 1-d integer array, got shape {a.shape}")
        if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):
            raise ValueError(f"{what} must be integers, got {a.dtype}")
        return a.astype(np.int64)
    st, ln = ints(starts, "starts"), ints(lengths, "lengths")
    if st.shape != ln.shape:
        raise ValueError(f"starts and lengths differ in length: {st.size} != {ln.size}")
    if st.size == 0:
        return st, ln
    if (st < 0).any():
        raise ValueError(f"span {int(np.argmax(st < 0))} starts at {int(st[st < 0][0])}: starts must be >= 0")
    short = ln < min_samples_
    if short.any():
        raise ValueError(f"segment of {int(ln[short][0])} samples is too short: ECAPA's reflect padding needs at least "
                         f"{min_frames_} frames ({min_samples_} samples)")
    past = st + ln > n_total
    if past.any():
        i = int(np.argmax(past))
        raise ValueError(f"span {i} = [{int(st[i])}, {int(st[i] + ln[i])}) runs past the end of the signal ({n_total} samples)")
    return st, ln


def _np(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float32)


def _pad_to(v: int, m: int) -> int:
    return (v + m - 1) // m * m


K_ALIGN_F16 = 64  # K step of the f16 conv/GEMM kernel


def pack_conv_weight(w: np.ndarray, dtype=np.float32) -> np.ndarray:
    """[cout, cin, k] (torch Conv1d) -> [cout, k, cin_pad], zero padded (kernel layout);
    f32 with cin_pad % 32 == 0, or f16 with cin_pad % 64 == 0."""
    cout, cin, k = w.shape
    cin_pad = _pad_to(cin, K_ALIGN if dtype == np.float32 else K_ALIGN_F16)
    out = np.zeros((cout, k, cin_pad), dtype=dtype)
    out[:, :, :cin] = np.transpose(w, (0, 2, 1)).astype(dtype)
    return out


def split16_exponent(w: np.ndarray) -> int:
    """s with max |w| 2^s in [512, 1024) (0 for an all-zero tensor)."""
    wmax = float(np.abs(w).max())
    if not wmax > 0:
        return 0
    s = int(np.floor(np.log2(1024.0 / wmax)))
    return s - 1 if wmax * 2.0 ** s >= 1024.0 else s


def pack_conv_weight_split16(w: np.ndarray):
    """[cout, cin, k] f32 -> (SD_DT_SPLIT16 [cout, k, cin_pad / 32, 64] f16, s): the weights scaled by 2^s (max |w| 2^s in
    [512, 1024): the low halves of small weights stay clear of the f16 subnormals, nothing overflows), every value split
    hi = f16(v), lo = f16(v - hi), interleaved per 32 input channels [hi x 32 | lo x 32] (sd_hip.h: SD_DT_SPLIT16)."""
    cout, cin, k = w.shape
    cp = _pad_to(cin, 32)
    s = split16_exponent(w)
    v = np.zeros((cout, k, cp), dtype=np.float32)
    v[:, :, :cin] = np.transpose(w, (0, 2, 1)) * np.float32(2.0 ** s)          # exact: power of two
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    out = np.empty((cout, k, cp // 32, 64), dtype=np.float16)
    out[..., :32] = hi.reshape(cout, k, cp // 32, 32)
    out[..., 32:] = lo.reshape(cout, k, cp // 32, 32)
    return out, s


def bn_affine(sd: dict, prefix: str):
    g, b = _np(sd[f"{prefix}.weight"]), _np(sd[f"{prefix}.bias"])
    rm, rv = _np(sd[f"{prefix}.running_mean"]), _np(sd[f"{prefix}.running_var"])
    scale = (g.astype(np.float64) / np.sqrt(rv.astype(np.float64) + BN_EPS))
    shift = b.astype(np.float64) - rm.astype(np.float64) * scale
    return scale.astype(np.float32), shift.astype(np.float32)


def fold_constant_rows(w: np.ndarray, bias: np.ndarray, affine):
    """A conv + ReLU + BatchNorm layer whose output row r has no weight at all (a pruned or dead channel of a trained checkpoint) stores
    the constant relu(bias[r]) * scale[r] + shift[r] on every frame.  The column statistics of the conv epilogues sum y - shift
    (sd_hip.h: the one-pass form about the pivot), which for such a row is the constant relu(bias) * scale: its variance
    q / T - m^2 then cancels to about 1e-7 m^2 instead of 0, and the pooling's global std came out as 3e-4 |m| where speechbrain
    clamps to 1e-6.  Moving the constant into the shift (bias 0, shift + relu(bias) * scale, float64 on the host) stores the same
    value and makes every term of the sums exactly 0.  -> (bias, (scale, shift)); the inputs when no row is empty."""
    dead = ~np.any(w.reshape(w.shape[0], -1) != 0, axis=1)
    if not dead.any():
        return bias, affine
    scale, shift = affine
    bias, shift = bias.astype(np.float32, copy=True), shift.astype(np.float64)
    shift[dead] += np.maximum(bias[dead].astype(np.float64), 0.0) * scale[dead].astype(np.float64)
    bias[dead] = 0.0
    return bias, (scale, shift.astype(np.float32))


class EcapaWeights:
    """ECAPA-TDNN weights packed for the HIP kernels and resident on one device."""

    def __init__(self, state_dict: dict, device: torch.device, precision: str = "f32"):
        if precision not in ("f32", "f16", "f32s", "f32ns"):
            raise ValueError(f"precision must be 'f32', 'f16', 'f32s' (f32-split16x3) or 'f32ns' (exact-f32 wide layers, split16x3 narrow ones), got {precision!r}")
        self.device = device
        self.precision = precision
        self.split_narrow = True      # f32s: also the narrow convs on the split kernel (False: wide layers only, as first built)
        self.cfg: EcapaConfig = config_from_state_dict(state_dict)
        cfg = self.cfg
        if len(set(cfg.channels[:-1])) != 1 or cfg.channels[-1] != cfg.n_blocks * cfg.channels[0]:
            raise ValueError(f"unsupported ECAPA geometry {cfg.channels}: blocks must share one width and MFA = n_blocks * width")
        self._keep: list[torch.Tensor] = []
        sd = state_dict
        W = N.sd_ecapa_weights()
        W.w_dtype = N.SD_DT_F16 if precision == "f16" else N.SD_DT_F32
        W.split16 = {"f32s": 1, "f32ns": 2}.get(precision, 0)      # 2: only the narrow layers carry the split packing
        W.n_mels = cfg.input_size
        W.channels = cfg.channels[0]
        W.n_blocks = cfg.n_blocks
        W.res2_scale = cfg.res2net_scale
        W.mfa_channels = cfg.channels[-1]
        W.att_channels = cfg.attention_channels
        W.emb_dim = cfg.lin_neurons
        W.asp_eps = 1e-12
        self._fill(W.block0, _np(sd["blocks.0.conv.conv.weight"]), _np(sd["blocks.0.conv.conv.bias"]),
                   bn_affine(sd, "blocks.0.norm.norm"), cfg.dilations[0])
        for i in range(1, cfg.n_blocks + 1):
            blk = W.blocks[i - 1]
            p = f"blocks.{i}"
            d = cfg.dilations[i]
            self._fill(blk.tdnn1, _np(sd[f"{p}.tdnn1.conv.conv.weight"]), _np(sd[f"{p}.tdnn1.conv.conv.bias"]),
                       bn_affine(sd, f"{p}.tdnn1.norm.norm"), 1)
            for j in range(cfg.res2net_scale - 1):
                q = f"{p}.res2net_block.blocks.{j}"
                self._fill(blk.res2[j], _np(sd[f"{q}.conv.conv.weight"]), _np(sd[f"{q}.conv.conv.bias"]),
                           bn_affine(sd, f"{q}.norm.norm"), d)
            self._fill(blk.tdnn2, _np(sd[f"{p}.tdnn2.conv.conv.weight"]), _np(sd[f"{p}.tdnn2.conv.conv.bias"]),
                       bn_affine(sd, f"{p}.tdnn2.norm.norm"), 1)
            self._fill(blk.se1, _np(sd[f"{p}.se_block.conv1.conv.weight"]), _np(sd[f"{p}.se_block.conv1.conv.bias"]), None, 1, per_segment=True)
            self._fill(blk.se2, _np(sd[f"{p}.se_block.conv2.conv.weight"]), _np(sd[f"{p}.se_block.conv2.conv.bias"]), None, 1, per_segment=True)
        self._fill(W.mfa, _np(sd["mfa.conv.conv.weight"]), _np(sd["mfa.conv.conv.bias"]), bn_affine(sd, "mfa.norm.norm"), 1)
        cm = cfg.channels[-1]
        wa = _np(sd["asp.tdnn.conv.conv.weight"])  # [att, 3*cm, 1] acting on cat(h, mean, std)
        self._fill(W.asp_tdnn_h, wa[:, :cm], None, bn_affine(sd, "asp.tdnn.norm.norm"), 1)
        self._fill(W.asp_tdnn_g, wa[:, cm:], _np(sd["asp.tdnn.conv.conv.bias"]), None, 1, per_segment=True)
        self._fill(W.asp_conv, _np(sd["asp.conv.conv.weight"]), _np(sd["asp.conv.conv.bias"]), None, 1)
        if precision in ("f32s", "f32ns"):      # the fused pooling kernel splits these f32 weights in registers: it needs their 2^s
            W.asp_conv.split_scale_inv = float(2.0 ** -split16_exponent(_np(sd["asp.conv.conv.weight"])))
        # asp_bn is an affine map in front of a linear layer: fold it into fc (float64 on the host)
        s, t = bn_affine(sd, "asp_bn.norm")
        wf = _np(sd["fc.conv.weight"]).astype(np.float64)[:, :, 0]
        bf = _np(sd["fc.conv.bias"]).astype(np.float64)
        w_fold = (wf * s.astype(np.float64)[None, :]).astype(np.float32)[:, :, None]
        b_fold = (bf + wf @ t.astype(np.float64)).astype(np.float32)
        self._fill(W.fc, w_fold, b_fold, None, 1, per_segment=True)
        self.struct = W
        self.n_params = sum(int(np.prod(v.shape)) for k, v in sd.items() if "running" not in k and "num_batches" not in k)

    def _dev(self, a: np.ndarray, dtype=np.float32) -> int:
        t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.device)
        self._keep.append(t)
        return t.data_ptr()

    def _fill(self, L, w: np.ndarray, bias, affine, dil: int, per_segment: bool = False) -> None:
        """Frame-level layers (M = B*T rows) follow the engine precision; per-segment layers
        (M = B rows: SE gate, global-context bias, FC) always stay f32."""
        cout, cin, k = w.shape
        if affine is not None and bias is not None:        # the conv + ReLU + BatchNorm layers (every layer the forward runs with an affine and its own bias)
            bias, affine = fold_constant_rows(w, bias, affine)
        half = self.precision == "f16" and not per_segment
        wdt = np.float16 if half else np.float32
        if half and not float(np.abs(w).max()) < 65520.0:        # 65520 and above round to inf
            # the f16 mode casts the weights unscaled: beyond the f16 range they would reach the matrix cores as inf (NaN keeps refusing too)
            raise ValueError(f"precision 'f16': a frame-level conv weight {cout}x{cin}x{k} holds max |w| = {float(np.abs(w).max()):.4g}, which "
                             f"f16 cannot hold (65504); use precision 'f32', 'f32s' or 'f32ns' for this checkpoint")
        packed = pack_conv_weight(w, wdt)
        L.w = self._dev(packed, wdt)
        L.w_dtype = N.SD_DT_F16 if half else N.SD_DT_F32
        L.bias = self._dev(bias) if bias is not None else None
        if affine is not None:
            L.scale, L.shift = self._dev(affine[0]), self._dev(affine[1])
        else:
            L.scale, L.shift = None, None
        L.cin, L.cin_pad, L.cout, L.taps, L.dil = cin, packed.shape[2], cout, k, dil
        # "f32s": the frame-level conv layers get a second, split-f16 packing.  Wide outputs (stem, tdnn1, tdnn2, MFA: 86 % of
        # the flops; 256x256 kernel, SD_DT_SPLIT16 activations) carry the weight scale 2^s in bias * 2^s / scale * 2^-s; narrow
        # ones (Res2Net convs, attention TDNN; 128x128 kernel that splits f32 activations while staging) pass 2^-s to the kernel
        L.w_split, L.bias_split, L.scale_split, L.split_scale_inv = None, None, None, 0.0
        if self.precision in ("f32s", "f32ns") and not per_segment and cin % 4 == 0:
            if self.precision == "f32s" and cout >= 1024 and affine is not None and bias is not None:
                ws, s = pack_conv_weight_split16(w)
                L.w_split = self._dev(ws, np.float16)
                L.bias_split = self._dev(bias * np.float32(2.0 ** s))
                L.scale_split = self._dev(affine[0] * np.float32(2.0 ** -s))
            elif cout <= 256 and self.split_narrow:
                ws, s = pack_conv_weight_split16(w)
                L.w_split = self._dev(ws, np.float16)
                L.split_scale_inv = float(2.0 ** -s)


def forward_entries(precision: str) -> tuple[str, str]:
    """(forward, forward with relative lengths): the entries an engine of `precision` calls.  "f32s" / "f32ns" are a property of the
    packed weights (sd_ecapa_weights.split16) on the f32 schedule, so they share the f32 entries."""
    if precision == "f16":
        return "sd_ecapa_forward_f16", "sd_ecapa_forward_lens_f16"
    return "sd_ecapa_forward_f32", "sd_ecapa_forward_lens_f32"


class EmbeddingEngine:
    """fbank + ECAPA-TDNN on one GPU. Thread-safe (one forward at a time per engine)."""

    def __init__(self, state_dict: dict, device="cuda", max_batch: int = 512, precision: str = "f32"):
        self.device = torch.device(device if not isinstance(device, int) else f"cuda:{device}")
        if self.device.type != "cuda":
            raise RuntimeError(f"EmbeddingEngine runs on the GPU only (got device {self.device}); there is no CPU fallback")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._lib = N.load()
        self.max_batch = int(max_batch)
        self._lock = threading.Lock()
        with torch.cuda.device(self.device):
            self.weights = EcapaWeights(state_dict, self.device, precision)
            self.plan = FbankPlan("speechbrain", n_mels=self.weights.cfg.input_size)
        self.dim = self.weights.cfg.lin_neurons
        self.min_samples = min_samples(self.weights.cfg)
        self.precision = precision
        # "f32s" = f32-split16x3: the f32 schedule (f32 activations) whose wide layers run three f16 MFMA products per value pair at
        # f32-level accuracy
        self._forward, self._forward_lens = forward_entries(precision)
        self._ws = None
        self._ws_frozen = False

    # -- workspace: feats + fbank scratch + ECAPA activations, three flat buffers that only ever grow (keyed by
    # capacity, not by the exact (B, n): the reference's callers send batches whose padded length changes every call
    # [REF anti_stick_diarize.py:163-166], and re-allocating ~10 MB per segment per call was a measurable part of it)
    # Sized once per call for the largest micro-batch; the shorter last one runs in the same buffers: the sizing functions never shrink
    # as B grows (tests/test_buffer_rules.py)
    def _workspace(self, B: int, n: int):
        T = FbankPlan.num_frames(n)
        n_mels = self.weights.cfg.input_size
        return self._grow((B * T * n_mels * 4, max(self.plan.workspace_bytes(B, n), 256),
                           int(self._lib.sd_ecapa_workspace_bytes(C.byref(self.weights.struct), B, T))))

    def _packed_workspace(self, B: int, M: int, n_max: int):
        n_mels = self.weights.cfg.input_size
        return self._grow((M * n_mels * 4, max(self.plan.packed_workspace_bytes(B, M, n_max), 256),
                           int(self._lib.sd_ecapa_packed_workspace_bytes(C.byref(self.weights.struct), B, M))))

    def _grow(self, need):
        if self._ws is None:
            self._ws = [None, None, None]
        for i, nbytes in enumerate(need):
            if self._ws[i] is None or self._ws[i].numel() < nbytes:
                if self._ws_frozen:
                    raise RuntimeError("this engine's workspace is referenced by a captured hipGraph (StreamingEmbedder); "
                                       "use a separate EmbeddingEngine for larger batches")
                self._ws[i] = None                     # release before growing
                self._ws[i] = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        return self._ws

    def sibling(self) -> "EmbeddingEngine":
        """A second engine over the SAME packed weights and fbank tables (read-only on the device) with a workspace and a lock of
        its own: two siblings can run forwards on two streams at once (`HipEcapaEncoder.encode_batches`)."""
        other = object.__new__(EmbeddingEngine)
        other.__dict__.update(self.__dict__)
        other._lock = threading.Lock()
        other._ws = None
        other._ws_frozen = False
        return other

    def freeze_workspace(self) -> None:
        """After a hipGraph capture of `embed`: the captured launches hold the workspace pointers, so it may no longer move."""
        self._ws_frozen = True

    def embed(self, wav: torch.Tensor, rel_lens: torch.Tensor | None = None) -> torch.Tensor:
        """wav: f32 [B, n] on this engine's device -> f32 [B, dim] on the device (async on the current stream).
        rel_lens (optional): speechbrain's relative lengths, f32 [B] on the device (validated by the caller: encode_batch);
        the fbank mean and the SE / pooling statistics then count each row's leading frames only (include/sd_hip.h,
        "Relative lengths").  The counts come from T of the padded n, so micro-batching does not change them."""
        if wav.dim() != 2:
            raise AssertionError("wav must be [B, n]")
        if wav.device != self.device:
            raise ValueError(f"wav is on {wav.device}, engine on {self.device}")
        wav = wav.contiguous().float()
        B, n = wav.shape
        if rel_lens is not None:
            if rel_lens.shape != (B,) or rel_lens.dtype != torch.float32 or rel_lens.device != self.device:
                raise ValueError(f"rel_lens must be f32 [{B}] on {self.device}, got {rel_lens.dtype} {tuple(rel_lens.shape)} on {rel_lens.device}")
            rel_lens = rel_lens.contiguous()
        out = torch.empty((B, self.dim), dtype=torch.float32, device=self.device)
        if B == 0:
            return out
        if n < self.min_samples:
            raise ValueError(f"segment of {n} samples is too short: ECAPA's reflect padding needs at least "
                             f"{min_frames(self.weights.cfg)} frames ({self.min_samples} samples)")
        with self._lock:
            mb = min(self.max_batch, B)
            feats, fb_ws, ec_ws = self._workspace(mb, n)
            T = FbankPlan.num_frames(n)
            W = C.byref(self.weights.struct)
            for lo in range(0, B, mb):
                nb = min(mb, B - lo)
                x = wav[lo:lo + nb]
                rl = None if rel_lens is None else rel_lens[lo:lo + nb]
                self.plan.rows(x, feats, fb_ws, rl)
                y = out[lo:lo + nb].data_ptr()
                if rl is not None:
                    ops.launch(self._forward_lens, x, W, feats.data_ptr(), nb, T, rl.data_ptr(), y, ec_ws.data_ptr(), ec_ws.numel())
                else:
                    ops.launch(self._forward, x, W, feats.data_ptr(), nb, T, y, ec_ws.data_ptr(), ec_ws.numel())
        return out

    def embed_windows(self, signal: torch.Tensor, starts: torch.Tensor, n: int) -> torch.Tensor:
        """Embeddings of the B windows `signal[starts[b] : starts[b] + n]` of ONE recording (zeros where a window hangs
        over an end of the signal), without gathering them: `sd_fbank_windows_f32` reads the resident signal at
        `starts[b]`, so the recording crosses PCIe once and no [B, n] matrix is written to and re-read from HBM.
        Bitwise `embed(gathered windows)`.  signal: f32 [n_total] on the device; starts: int64 [B] (any device);
        -> f32 [B, dim] on the device.  [REF anti_stick_diarize.py:82-100, 396-430]: the callers' window loops."""
        if signal.dim() != 1:
            raise AssertionError("signal must be [n_total]")
        if signal.device != self.device:
            raise ValueError(f"signal is on {signal.device}, engine on {self.device}")
        signal = signal.contiguous().float()
        starts = starts.to(self.device, dtype=torch.int64).contiguous()
        B, n = int(starts.numel()), int(n)
        out = torch.empty((B, self.dim), dtype=torch.float32, device=self.device)
        if B == 0:
            return out
        if n < self.min_samples:
            raise ValueError(f"window of {n} samples is too short: ECAPA's reflect padding needs at least "
                             f"{min_frames(self.weights.cfg)} frames ({self.min_samples} samples)")
        if signal.numel() < 1:
            raise ValueError("empty signal")
        with self._lock:
            mb = min(self.max_batch, B)
            feats, fb_ws, ec_ws = self._workspace(mb, n)
            T = FbankPlan.num_frames(n)
            W = C.byref(self.weights.struct)
            for lo in range(0, B, mb):
                nb = min(mb, B - lo)
                self.plan.windows(signal, starts[lo:lo + nb], n, feats, fb_ws)
                ops.launch(self._forward, signal, W, feats.data_ptr(), nb, T, out[lo:lo + nb].data_ptr(), ec_ws.data_ptr(), ec_ws.numel())
        return out

    def embed_spans(self, signal: torch.Tensor, starts, lengths, frame_budget: int | None = None) -> torch.Tensor:
        """Embeddings of the B spans `signal[starts[s] : starts[s] + lengths[s]]` of ONE recording, each as if it were embedded alone
        (`embed(span[None])` up to f32 rounding), with no padding to the longest: the spans' frames are packed back to back
        (`sd_fbank_packed_f32` + `sd_ecapa_forward_packed_f32`, include/sd_hip.h "Packed spans").  Exact f32 only.
        signal: f32 [n_total] on this engine's device; starts, lengths: integer arrays [B] (host or device) -> f32 [B, dim] on the
        device.  Micro-batches of consecutive spans up to `frame_budget` frames (default max_batch x 201); a span is never split.
        Everything is validated before the first launch."""
        if self.precision != "f32":
            raise NotImplementedError(f"embed_spans runs the exact-f32 schedule only (precision 'f32'); this engine is {self.precision!r}")
        if not isinstance(signal, torch.Tensor) or signal.dim() != 1 or signal.dtype != torch.float32:
            raise ValueError("signal must be a 1-d f32 tensor")
        if signal.device != self.device:
            raise ValueError(f"signal is on {signal.device}, engine on {self.device}")
        st, ln = check_spans(starts, lengths, int(signal.numel()), self.min_samples, min_frames(self.weights.cfg))
        budget = self.max_batch * SPAN_BUDGET_FRAMES if frame_budget is None else int(frame_budget)
        if budget < 1:
            raise ValueError(f"frame_budget must be positive, got {frame_budget}")
        B = int(st.size)
        out = torch.empty((B, self.dim), dtype=torch.float32, device=self.device)
        if B == 0:
            return out
        signal = signal.contiguous()
        frames = 1 + ln // HOP
        batches = plan_span_batches(frames, budget)
        # one upload of every table: starts, lengths and each micro-batch's own frame offsets (from 0) back to back
        offs = [span_frame_offsets(ln[lo:hi]) for lo, hi in batches]
        fs_at = np.concatenate([[0], np.cumsum([o.size for o in offs])])
        host = torch.from_numpy(np.concatenate([st, ln, np.concatenate(offs)]).astype(np.int64))
        tab = host.to(self.device)
        st_d = tab[:B]
        ln_d = tab[B:2 * B].to(torch.int32)
        fs_d = tab[2 * B:].to(torch.int32)
        W = C.byref(self.weights.struct)
        with self._lock:
            for (lo, hi), o, f0 in zip(batches, offs, fs_at[:-1]):
                nb, M, n_max = hi - lo, int(o[-1]), int(ln[lo:hi].max())
                feats, fb_ws, ec_ws = self._packed_workspace(nb, M, n_max)
                fs = fs_d[int(f0):int(f0) + nb + 1]
                self.plan.packed(signal, st_d[lo:hi], ln_d[lo:hi], fs, M, n_max, feats, fb_ws)
                ops.launch("sd_ecapa_forward_packed_f32", signal, W, feats.data_ptr(), fs.data_ptr(), nb, M, out[lo:hi].data_ptr(), ec_ws.data_ptr(),
                           ec_ws.numel())
        return out

    def features(self, wav: torch.Tensor) -> torch.Tensor:
        """The mean-normalised fbank the network consumes, [B, T, n_mels] (diagnostics / tests)."""
        wav = wav.contiguous().float()
        B, n = wav.shape
        return fbank_device(wav, self.plan, mean_norm=True)


def fbank_windows_device(signal: torch.Tensor, starts: torch.Tensor, n: int, plan: FbankPlan, mean_norm: bool = True) -> torch.Tensor:
    """HIP fbank of the windows signal[starts[b] : starts[b] + n] of one device-resident recording -> [B, T, n_mels]."""
    if signal.dim() != 1 or signal.device.type != "cuda":
        raise RuntimeError("fbank_windows_device needs a 1-d GPU tensor; there is no CPU fallback")
    signal = signal.contiguous().float()
    starts = starts.to(signal.device, dtype=torch.int64).contiguous()
    B = int(starts.numel())
    T = plan.frames(int(n))
    out = torch.empty((B, T, plan.n_mels), dtype=torch.float32, device=signal.device)
    if B == 0:
        return out
    ws = torch.empty((max(plan.workspace_bytes(B, n), 256),), dtype=torch.uint8, device=signal.device)
    plan.windows(signal, starts, n, out, ws, mean_norm)
    return out


def fbank_packed_device(signal: torch.Tensor, starts, lengths, plan: FbankPlan) -> torch.Tensor:
    """HIP fbank (mean-normalised) of the packed spans signal[starts[s] : starts[s] + lengths[s]] of one device-resident recording
    -> [M, n_mels], span s at rows frame_start[s] .. frame_start[s + 1] (`span_frame_offsets`)."""
    if signal.dim() != 1 or signal.device.type != "cuda":
        raise RuntimeError("fbank_packed_device needs a 1-d GPU tensor; there is no CPU fallback")
    signal = signal.contiguous().float()
    st, ln = check_spans(starts, lengths, int(signal.numel()), 1, 1)
    fs = span_frame_offsets(ln)
    B, M = int(st.size), int(fs[-1])
    out = torch.empty((M, plan.n_mels), dtype=torch.float32, device=signal.device)
    if B == 0:
        return out
    st_d = torch.from_numpy(st).to(signal.device)
    ln_d = torch.from_numpy(ln.astype(np.int32)).to(signal.device)
    fs_d = torch.from_numpy(fs).to(signal.device)
    n_max = int(ln.max())
    ws = torch.empty((max(plan.packed_workspace_bytes(B, M, n_max), 256),), dtype=torch.uint8, device=signal.device)
    plan.packed(signal, st_d, ln_d, fs_d, M, n_max, out, ws)
    return out


def fbank_device(wav: torch.Tensor, plan: FbankPlan, mean_norm: bool = True) -> torch.Tensor:
    """Run the HIP fbank on a device tensor [B, n] -> [B, T, n_mels]."""
    if wav.dim() != 2:
        raise AssertionError("wav must be [B, n]")
    if wav.device.type != "cuda":
        raise RuntimeError("fbank_device needs a GPU tensor; there is no CPU fallback")
    wav = wav.contiguous().float()
    B, n = wav.shape
    T = plan.frames(n)
    out = torch.empty((B, T, plan.n_mels), dtype=torch.float32, device=wav.device)
    if B == 0:
        return out
    ws = torch.empty((max(plan.workspace_bytes(B, n), 256),), dtype=torch.uint8, device=wav.device)
    plan.rows(wav, out, ws, mean_norm=mean_norm)
    return out
