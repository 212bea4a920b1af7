"""Trained-like ECAPA state dicts: the WEIGHT axis of the suite.  TEST INFRASTRUCTURE; nothing under speech-diarization_amd/ imports it.

Every other test takes its network from `synth.make_ecapa_state_dict`: Gaussian conv weights of std 1 / sqrt(fan in), BatchNorm weights
and variances in [0.5, 1.5].  A trained checkpoint cannot be loaded here, so `trained_like_state_dict` builds the features one has and the
init lacks, in two steps.

SHAPE, from `make_ecapa_state_dict(seed, config(geom))`, every draw from synth's counter-based streams (tags "tl.<key>..."):
  * every conv weight times exp(tail z), z standard normal per element, rescaled to the tensor's former std.  max / rms of a tensor of
    n values is at most sqrt(n), so what a tail gives depends on the tensor: at tail 2.0 60 to 220 for the tensors of 16384 values and
    more (1000 at the full width), 10 to 50 for the 16 x 16 x 3 Res2Net convs of width 128; at tail 1.0 a quarter of that;
  * ZERO_ROWS = 2 % of the output rows of every conv (at least one) exactly zero;
  * asp.conv times ATT_GAIN = 40: attention logits tens wide over a segment (median 6 to 17, the widest several hundred), and
    max |w| of 296 (w256a128) and 1440 (full), so that the fused split pooling needs the layer's own 2^s (a fixed 2^8 overflows f16
    from |w| = 256 on) and, at the full width, a NEGATIVE s.  At 32 the w256a128 maximum is 237 and a fixed 2^8 would still do;
  * +BIAS_SHIFT = 3 on 10 % and -3 on another 10 % of the biases of the frame-level convs (always-on / always-off channels behind the
    ReLU); the SE and fc biases as they are;
  * the BatchNorm weight negated on NEG_GAMMA = 10 % of the channels and times 1e-3 on another TINY_GAMMA = 5 % (at least one each), its
    bias times BETA_GAIN = 5.
CALIBRATE: one float64 forward of an `EcapaRef` whose `_bn` writes the mean and the variance over batch and time of its input, the
variance floored at VAR_FLOOR = 0.1, into running_mean / running_var before it applies them; `_bn` is called layer by layer, so one
forward calibrates the whole net, asp_bn included.  Without a floor an always-off channel has variance 0 and a scale of 316 gamma.

The calibration inputs are N_CALIB = 10 two-second windows (hop 2.2 s) of `synth.synthetic_conversation(24.0, 3, seed=5)` through
`fbank_ref.speechbrain_fbank_ref`: the front end the engine runs, in dB.  (`fbank_batch_ref` is in ln, 4.3 times smaller; a net
calibrated on it sees four times its statistics when the engine evaluates it.)  The evaluation inputs (`eval_wav`) are windows of the
same recording at other offsets.

Why these values and no others, each against the conditions of tests/test_weight_axis_rules.py at width 128 (float64 and float32 oracle):
  * six windows or a floor of 1e-2: a channel that is off in every calibration frame and on in an evaluation frame is amplified by
    gamma / sqrt(floor) = 10 gamma, once per block along the residual path; depending on where the evaluation windows start (the
    sentence mean of a window moves by 20 dB with its share of silence) the largest activation was 1000 to 7900, against the 2^11 that
    f16 storage allows.  With 0.1 it is 9 to 43 for three different sets of offsets, at both tails;
  * ATT_GAIN = 40 with the floor of 0.1: the f32 oracle (f32 fbank included) sits 3e-12 to 4.3e-10 (cosine) from float64, against
    6e-14 at the init weights and a condition of 1e-9; at 64 the worst case (tail 1.0, 2 s windows) is 1.3e-9, at 48 7e-10.
    Different segments are 0.25 to 1.0 apart; 10 % of the MFA channels are constant over time.
Returns f32 arrays, as a checkpoint holds."""
import functools

import numpy as np
import torch

from oracle.ecapa_ref import EcapaRef
from oracle.fbank_ref import speechbrain_fbank_ref
from speech_diarization_amd import synth

import ecapa_plan as P

ZERO_ROWS, NEG_GAMMA, TINY_GAMMA, TINY, BIAS_UP, BIAS_DOWN, BIAS_SHIFT, BETA_GAIN, VAR_FLOOR = 0.02, 0.10, 0.05, 1e-3, 0.10, 0.10, 3.0, 5.0, 0.1
ATT_GAIN = 40.0
N_CALIB, CALIB_HOP, WINDOW = 10, 35200, 32000
EVAL_FIRST, EVAL_HOP = 20000, 61000
PARAMS = dict(zero_rows=ZERO_ROWS, neg_gamma=NEG_GAMMA, tiny_gamma=TINY_GAMMA, tiny=TINY, bias_up=BIAS_UP, bias_down=BIAS_DOWN,
              bias_shift=BIAS_SHIFT, beta_gain=BETA_GAIN, att_gain=ATT_GAIN, var_floor=VAR_FLOOR, eval_first=EVAL_FIRST, eval_hop=EVAL_HOP,
              n_calib=N_CALIB, calib_hop=CALIB_HOP, window=WINDOW,
              recording="synthetic_conversation(24.0, 3, seed=5)", front_end="speechbrain_fbank_ref")


config = P.config           # "w128", "w256a128", "full": the geometries of tests/helpers/ecapa_plan.py


@functools.lru_cache(maxsize=None)
def recording():
    return synth.synthetic_conversation(24.0, 3, seed=5).wav


def calib_wav():
    y = recording()
    return np.stack([y[i * CALIB_HOP: i * CALIB_HOP + WINDOW] for i in range(N_CALIB)])


def eval_wav(B, n):
    """B windows of n samples that are no calibration window: offsets 20000 + 61000 b (three voices, turns of 3 to 6 s)."""
    y = recording()
    return np.stack([y[EVAL_FIRST + EVAL_HOP * b: EVAL_FIRST + EVAL_HOP * b + n] for b in range(B)])


def conv_keys(sd):
    return [k for k in sd if k.endswith("conv.weight")]


def bn_prefixes(sd):
    return [k[:-len(".running_var")] for k in sd if k.endswith(".running_var")]


def is_frame_level(key):
    """A conv whose rows are frames: everything but the SE pair and fc (per-segment layers, which `EcapaWeights._fill` keeps f32)."""
    return ".se_block." not in key and not key.startswith("fc.")


def picks(seed, tag, n, *shares):
    """Disjoint index sets of round(share n) (at least one) members each, from one permutation drawn from (seed, tag)."""
    order = np.argsort(synth._stream(seed, tag, n, 0), kind="stable")
    out, at = [], 0
    for share in shares:
        m = max(1, int(round(share * n)))
        out.append(order[at: at + m])
        at += m
    return out


def shaped_state_dict(geom, seed, tail):
    sd = {k: np.array(v, copy=True) for k, v in synth.make_ecapa_state_dict(seed, config(geom)).items()}
    for key in conv_keys(sd):
        w = sd[key].astype(np.float64)
        std = w.std()
        w = w * np.exp(tail * synth.normal(seed, f"tl.{key}.z", w.shape).astype(np.float64))
        w *= std / w.std()
        (rows,) = picks(seed, f"tl.{key}.rows", w.shape[0], ZERO_ROWS)
        w[rows] = 0.0
        if key == "asp.conv.conv.weight":
            w *= ATT_GAIN
        sd[key] = w.astype(np.float32)
        if is_frame_level(key):
            bkey = key[:-len("weight")] + "bias"
            up, down = picks(seed, f"tl.{bkey}", w.shape[0], BIAS_UP, BIAS_DOWN)
            b = sd[bkey].astype(np.float64)
            b[up] += BIAS_SHIFT
            b[down] -= BIAS_SHIFT
            sd[bkey] = b.astype(np.float32)
    for bn in bn_prefixes(sd):
        g = sd[f"{bn}.weight"].astype(np.float64)
        neg, tiny = picks(seed, f"tl.{bn}.g", len(g), NEG_GAMMA, TINY_GAMMA)
        g[neg] *= -1.0
        g[tiny] *= TINY
        sd[f"{bn}.weight"] = g.astype(np.float32)
        sd[f"{bn}.bias"] = (sd[f"{bn}.bias"].astype(np.float64) * BETA_GAIN).astype(np.float32)
    return sd


class CalibratingRef(EcapaRef):
    """float64 `EcapaRef` whose BatchNorm takes its statistics from the batch it is shown (floored variance) and keeps them."""

    def __init__(self, state_dict):
        super().__init__(state_dict, torch.float64)
        self.seen = {}

    def _bn(self, x, name):
        dims = (0, 2) if x.dim() == 3 else (0,)
        mean, var = x.mean(dim=dims), x.var(dim=dims, unbiased=False)
        self.seen[name] = (mean.reshape(-1).numpy().copy(), var.reshape(-1).numpy().copy())
        self.sd[f"{name}.norm.running_mean"] = mean.reshape(-1)
        self.sd[f"{name}.norm.running_var"] = var.reshape(-1).clamp(min=VAR_FLOOR)
        return super()._bn(x, name)


@functools.lru_cache(maxsize=None)
def calib_feats():
    return torch.from_numpy(speechbrain_fbank_ref(calib_wav()))


def trained_like_state_dict(geom, seed=1234, tail=2.0):
    """-> speechbrain-keyed dict of f32 arrays, a function of its arguments alone."""
    sd = shaped_state_dict(geom, seed, tail)
    net = CalibratingRef(sd)
    net.forward_features(calib_feats())
    for bn in bn_prefixes(sd):
        for stat in ("running_mean", "running_var"):
            sd[f"{bn}.{stat}"] = net.sd[f"{bn}.{stat}"].numpy().astype(np.float32)
    return sd


class RecordingRef(EcapaRef):
    """`EcapaRef` that keeps the mean and variance of every BatchNorm's input (the rules compare them with the dict's statistics)."""

    def __init__(self, state_dict, dtype=torch.float64):
        super().__init__(state_dict, dtype)
        self.seen = {}

    def _bn(self, x, name):
        dims = (0, 2) if x.dim() == 3 else (0,)
        self.seen[name] = (x.mean(dim=dims).reshape(-1).numpy().copy(), x.var(dim=dims, unbiased=False).reshape(-1).numpy().copy())
        return super()._bn(x, name)


def cos_dist(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


# ------------------------------------------------------------------ the references of one run: float64, float32, and f32 with f16 stores

def oracle64(sd, wav):
    from oracle import pipeline_ref
    return pipeline_ref.encode_batch_ref(sd, np.asarray(wav), torch.float64)


def oracle32(sd, wav):
    """The float32 oracle end to end (f32 torch fbank, f32 `EcapaRef`): what an f32 implementation in torch's summation order gives."""
    from oracle import pipeline_ref
    return pipeline_ref.encode_batch_ref(sd, np.asarray(wav), torch.float32)


def r16(x):
    return x.to(torch.float16).to(torch.float32)


class EmuF16Ref(EcapaRef):
    """float32 `EcapaRef` that rounds to f16 what the engine's f16 mode STORES as f16, and nothing else.  Read in
    speech-diarization_amd/csrc/sd_ecapa.hip (make_plan, with A = AS_F16) and engine.py (`EcapaWeights._fill`):
      * the weights of every frame-level conv (`_fill`: half = precision == "f16" and not per_segment): stem, tdnn1, Res2Net convs,
        tdnn2, MFA, asp.conv, and the h columns of asp.tdnn (`asp_tdnn_h`; its mean / std columns, `asp_tdnn_g`, are per-segment: f32);
      * the features, rounded once by the cast step in front of the stem ("the features are rounded to f16 once");
      * every frame-level layer's output after its whole epilogue (bias, ReLU, BatchNorm affine, tanh for the attention TDNN): x0, r,
        each Res2Net y_j, t2, h, a1 -- buffers of form A in the plan;
      * the Res2Net adds c_{j+1} + y_j (the tee of conv j, buffers s0 / s1 of form A; in the fused chain the f16 state in LDS);
      * the SE output gate * t2 + shortcut (se_scale writes slice i of xcat in form A).
    NOT rounded, as there: the SE squeeze, se1 / se2 and the gate (semean, seh, gate: AS_F32), the global mean / std (stats), the
    global-context bias, the attention logits (never stored by the fused pooling; f32 accumulators), the pooled statistics,
    asp_bn and fc -- everything with one row per segment."""

    def __init__(self, state_dict):
        super().__init__(state_dict, torch.float32)
        cm = self.sd["mfa.conv.conv.weight"].shape[0]
        for key in conv_keys(self.sd):
            if not is_frame_level(key):
                continue
            if key == "asp.tdnn.conv.conv.weight":
                self.sd[key] = torch.cat([r16(self.sd[key][:, :cm]), self.sd[key][:, cm:]], dim=1)
            else:
                self.sd[key] = r16(self.sd[key])

    def _tdnn16(self, x, name, dilation=1):
        return r16(self._tdnn(x, name, dilation))

    @torch.no_grad()
    def forward_features(self, feats):
        x = r16(feats.to(self.dtype)).transpose(1, 2)
        x = self._tdnn16(x, "blocks.0")
        xl = []
        for i in range(1, self.n_blocks + 1):
            p = f"blocks.{i}"
            residual = x
            t1 = self._tdnn16(x, f"{p}.tdnn1")
            ys = []
            for j, c in enumerate(torch.chunk(t1, self.scale, dim=1)):
                if j == 0:
                    y = c
                elif j == 1:
                    y = self._tdnn16(c, f"{p}.res2net_block.blocks.{j - 1}", i + 1)
                else:
                    y = self._tdnn16(r16(c + y), f"{p}.res2net_block.blocks.{j - 1}", i + 1)
                ys.append(y)
            t2 = self._tdnn16(torch.cat(ys, dim=1), f"{p}.tdnn2")
            s = t2.mean(dim=2, keepdim=True)
            s = torch.relu(self._conv(s, f"{p}.se_block.conv1"))
            s = torch.sigmoid(self._conv(s, f"{p}.se_block.conv2"))
            x = r16(s * t2 + residual)
            xl.append(x)
        h = self._tdnn16(torch.cat(xl, dim=1), "mfa")
        L = h.shape[2]
        mean = h.mean(dim=2)
        std = torch.sqrt(((h - mean.unsqueeze(2)) ** 2).mean(dim=2).clamp(min=1e-12))
        attn = torch.cat([h, mean.unsqueeze(2).expand(-1, -1, L), std.unsqueeze(2).expand(-1, -1, L)], dim=1)
        a1 = r16(torch.tanh(self._tdnn(attn, "asp.tdnn")))
        attn = torch.softmax(self._conv(a1, "asp.conv"), dim=2)
        mu = (attn * h).sum(dim=2)
        sd_ = torch.sqrt((attn * (h - mu.unsqueeze(2)) ** 2).sum(dim=2).clamp(min=1e-12))
        pooled = self._bn(torch.cat([mu, sd_], dim=1).unsqueeze(2), "asp_bn")
        return torch.nn.functional.conv1d(pooled, self.sd["fc.conv.weight"], self.sd["fc.conv.bias"]).squeeze(2)


def emu16(sd, wav):
    from oracle.fbank_ref import speechbrain_fbank_torch
    feats = speechbrain_fbank_torch(torch.from_numpy(np.asarray(wav, dtype=np.float32)))
    return EmuF16Ref(sd).forward_features(feats).numpy()


# (geometry, tail, B, samples) of the forward runs: tests/test_gpu_weights.py, tests/test_weight_axis_rules.py, tools/weight_axis.py.
# Width 128 at T = 61 and 201; w256a128, where the split modes launch their wide-role and fused forms; the full width at T = 129, the
# smallest T above the split column-statistics floor and the only case with cout >= 1024.
FORWARD_CASES = (("w128", 2.0, 3, 9600), ("w128", 2.0, 3, 32000), ("w128", 1.0, 3, 9600), ("w128", 1.0, 3, 32000),
                 ("w256a128", 2.0, 3, 32000), ("full", 2.0, 2, 20480))
SEED = 1234
FLOOR = {"f32": 1e-13, "f32ns": 1e-13, "f32s": 2e-13}        # the bars the precisions hold at the init weights (README.md, Magnitude)
F16_FLOOR = 2e-8


def bar(precision, d_ref32, d_emu16):
    """The bar of one run, per segment: 16 x the distance of the reference arithmetic of that precision at the same weights and inputs,
    plus the precision's bar at the init weights.  16 in cosine distance is 4 in error norm: 2 for an accumulation order that differs
    from torch's, 2 for the 2^-22 per product of the split forms against 2^-24."""
    if precision == "f16":
        return 16.0 * np.asarray(d_emu16) + F16_FLOOR
    return 16.0 * np.asarray(d_ref32) + FLOOR[precision]


def lens_wav(B, n, rel):
    """`eval_wav` rows zeroed past their relative length, as speechbrain's callers pad them -> (wav, f32 lengths)."""
    wav = eval_wav(B, n).copy()
    lens = np.asarray(rel, dtype=np.float32)
    for b in range(B):
        wav[b, int(np.ceil(lens[b] * n)):] = 0.0
    return wav, lens


def lens_oracle32(sd, wav, lens):
    """The float32 oracle under relative lengths: f32 torch fbank, the masked sentence mean in f32, `EcapaLensRef` in f32."""
    import wav_lens_ref as WL
    from oracle.fbank_ref import speechbrain_fbank_torch
    feats = speechbrain_fbank_torch(torch.from_numpy(np.asarray(wav, dtype=np.float32)), mean_norm=False)
    for b, k in enumerate(WL.sb_actual_sizes(lens, feats.shape[1])):
        feats[b] = feats[b] - feats[b, :k].mean(dim=0)
    return WL.EcapaLensRef(sd, torch.float32).forward_features(feats, torch.from_numpy(lens)).numpy()


SPANS = (640, 9600, 32000)


def span_signal():
    """(signal, starts): the spans back to back in one stretch of the recording."""
    starts = np.concatenate([[0], np.cumsum(SPANS)[:-1]])
    return recording()[EVAL_FIRST: EVAL_FIRST + int(sum(SPANS))].copy(), starts
