"""Known-answer cases for tests/test_exact_rules.py (CPU) and tests/test_gpu_exact.py: inputs on which every f32 product and sum
a kernel can form is exact (small integers, powers of two, one-hot weights), so that an int64 / float64 numpy reference gives
the BITS the kernel must produce, whatever its tile shape, K order, split-K order or MFMA form.

Every generator checks its own bit budget on the host and raises `BudgetError` when a case leaves it:
  * every value an f32 accumulator or an f32 epilogue can hold is below 2^24 in magnitude (bounded by sum |x| |w|, so the bound
    holds for every summation order) and is a multiple of a power of two that keeps it inside 24 bits;
  * every value stored as f16 survives the round trip through f16 and is at most 2048 in magnitude;
  * a mean divides by a power of two (or the quotient is an integer), quotient and square inside 24 bits.
A GPU mismatch on one of these cases is therefore never rounding.

Every generator also takes an exponent `e` (default 0: the case itself): the TWIN whose value operands -- x, bias and per-segment bias,
BN shift / colstat pivot, tee_add, the h of the pooling kernels, both inputs of se_scale_residual, eps by 4^e; never a weight, a scale,
a gate or a logit -- are times 2^e.  The operators are homogeneous of degree one in them, so the twin's answer is ldexp(answer, e), bit
for bit, and the budget is checked again on the scaled values: every f32 normal and exact, every f16 exact, subnormals included
(`F32_EXPONENTS`, `F16_EXPONENTS`; tests/test_gpu_scale.py, tests/test_scale_rules.py).  `split16_halves` / `split16_conv_sum` state the
arithmetic of the split operators (include/sd_hip.h) in numpy, for the twins whose halves are f16 subnormals.

`CASE_TABLE` names, for every case, the launch LABELS (include/sd_hip_trace.h: kernel, instantiation, walk) its runs reach on the
MI355X, and `F32_LABELS` / `f16_label` / `split_labels` the one label of each single run (case x selection x storage types x tuning);
tests/test_gpu_exact.py holds every run to its label through the launch log, so these are checked facts, not intentions.  Each entry
is derived from the dispatch rules of csrc/sd_conv_choice.h (`sd_choose_conv_f32`), sd_conv_gemm_f16.hip (`sd_conv1d_cl_f16`,
`sd_conv1d_cl_split16`), sd_pool.hip and sd_asp_fused.hip; the derivation stands beside it.  `EXACT_COVERAGE` is the inverse:
label -> cases."""
import functools
from dataclasses import dataclass

import numpy as np

F32_LIMIT = 1 << 24
F16_LIMIT = 2048
F16_MAX = 65504.0
# the exponents of the scaled twins: a case times 2^e must give the bits of ldexp(expected, e).  f32 storage: far from 1 both ways and
# still normal (eps 4^e as well); f16 storage (x, y, chain state, pooled h; the activations of the split operators, which are carried
# as f16 halves): +4 the top of the range, -14 astride the normal / subnormal edge, -20 mostly subnormal
F32_EXPONENTS = (-40, -12, 12, 40)
F16_EXPONENTS = (4, -14, -20)


class BudgetError(ValueError):
    """A case left the range in which its arithmetic is exact."""


def need_f32(name, *arrays, e=0):
    """Every value is an f32 below 2^24 in magnitude that survives the round trip (so: no rounding when it is formed).  `e`: the arrays
    are those of a twin scaled by 2^e (4^e: pass 2 e) -- divided by 2^e they meet the rule above, and as they stand every non-zero
    value is a NORMAL f32 that survives the round trip: normal and exact, so inside a 24-bit span."""
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        if not a.size:
            continue
        base = np.ldexp(a, -e)
        if np.abs(base).max() >= F32_LIMIT or not np.array_equal(base.astype(np.float32).astype(np.float64), base):
            raise BudgetError(f"{name}: a value leaves the exact f32 range (max |v| = {np.abs(base).max():g} times 2^{e})")
        with np.errstate(over="ignore"):
            back = a.astype(np.float32).astype(np.float64)
        if e and (not np.array_equal(back, a) or (np.abs(a[a != 0]) < 2.0 ** -126).any()):
            raise BudgetError(f"{name}: a value times 2^{e} is no normal f32")


def need_f16(name, *arrays, e=0):
    """Every value is an exact f16 of at most 2048; of a twin scaled by 2^e: an exact f16, subnormals included (a multiple of 2^-24),
    of at most 65504, whose unscaled value meets the rule above."""
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        if not a.size:
            continue
        base = np.ldexp(a, -e)
        if np.abs(base).max() > F16_LIMIT or not np.array_equal(base.astype(np.float16).astype(np.float64), base):
            raise BudgetError(f"{name}: a value is not an exact f16 of at most {F16_LIMIT} (max |v| = {np.abs(base).max():g})")
        with np.errstate(over="ignore"):
            back = a.astype(np.float16).astype(np.float64)
        if e and (np.abs(a).max() > F16_MAX or not np.array_equal(back, a)):
            raise BudgetError(f"{name}: a value times 2^{e} is no exact f16 (max |v| = {np.abs(a).max():g})")


def scaled(e, *arrays):
    """ldexp(a, e) of every array (None stays None): exact in float64 for every exponent used here."""
    out = tuple(None if a is None else np.ldexp(np.asarray(a, dtype=np.float64), e) for a in arrays)
    return out[0] if len(out) == 1 else out


def split16_halves(v, mul=1.0):
    """The header's statement of SD_DT_SPLIT16 in numpy: hi = f16(clamp(v mul)), lo = f16(v mul - hi), round to nearest even, f16
    subnormals kept (numpy's float16 has them).  -> (hi, lo) as float64."""
    v = np.clip(np.asarray(v, dtype=np.float32) * np.float32(mul), -F16_MAX, F16_MAX).astype(np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def split16_rows(v):
    """[M, C] f32 values -> the SD_DT_SPLIT16 rows sd_split16_pack_f32 must make of them: f16 [M, 2 C32], per 32 values
    [hi x 32 | lo x 32], the padding values zero."""
    M, Cc = np.shape(v)
    cp = -(-Cc // 32) * 32
    hi, lo = np.zeros((M, cp), np.float16), np.zeros((M, cp), np.float16)
    h, lw = split16_halves(v)
    hi[:, :Cc], lo[:, :Cc] = h, lw
    return np.concatenate([hi.reshape(M, cp // 32, 1, 32), lo.reshape(M, cp // 32, 1, 32)], axis=2).reshape(M, 2 * cp)


def split16_weight_shift(w):
    """The s of the weight pack: max |w| 2^s in [512, 1024) (engine.split16_exponent restated)."""
    top = float(np.abs(w).max())
    return 0 if top == 0 else 9 - int(np.floor(np.log2(top)))


def split16_conv_sum(x, w, src):
    """The three-product sum of sd_conv1d_cl_split16 in float64: x and w 2^s split into f16 halves, hi.hi + hi.lo + lo.hi over every
    tap and channel, times 2^-s; the lo.lo term dropped, as the kernel drops it."""
    s = split16_weight_shift(w)
    xh, xl = split16_halves(x)
    wh, wl = split16_halves(np.ldexp(np.asarray(w, dtype=np.float64), s))
    return np.ldexp(conv_sum(xh, wh, src) + conv_sum(xh, wl, src) + conv_sum(xl, wh, src), -s)


def need_mean(name, total, divisor):
    """total / divisor: the divisor a power of two (or the quotient an integer), quotient and its square inside 24 bits."""
    total = np.asarray(total, dtype=np.float64)
    q = total / divisor
    pow2 = divisor > 0 and (int(divisor) & (int(divisor) - 1)) == 0 and int(divisor) == divisor
    if not pow2 and not np.array_equal(q, np.round(q)):
        raise BudgetError(f"{name}: divisor {divisor} is no power of two and the quotient no integer")
    need_f32(name + " (mean)", q)
    need_f32(name + " (mean^2)", q * q)


# ------------------------------------------------------------------ conv shapes

# the shapes of the issue (what each crosses: the docstring of tests/test_gpu_exact.py).  H*: the same shapes for sd_conv1d_cl_f16, whose
# activations come in groups of 8 channels (S1's 36 channels are refused there: 40).  N128 / W*: the narrow and wide split16 forms.
SHAPES = {
    "S1": dict(B=3, T=57, cin=36, cout=72, k=3, dil=2),
    "S2": dict(B=2, T=131, cin=80, cout=1032, k=5, dil=1),
    "S3": dict(B=5, T=9, cin=128, cout=100, k=3, dil=4),
    "S4": dict(B=70, T=1, cin=544, cout=40, k=1, dil=1),
    "S5": dict(B=8, T=128, cin=32, cout=512, k=3, dil=2),        # fewer than 128 tiles of 128x128 but 128 of 64x64: the 64-row ring kernel
    "P": dict(spans=(5, 7, 5, 9, 131), cin=36, cout=72, k=3, dil=2),
    "H1": dict(B=3, T=57, cin=40, cout=72, k=3, dil=2),
    "H2": dict(B=2, T=131, cin=80, cout=1032, k=5, dil=1),
    "H2w": dict(B=2, T=131, cin=80, cout=1100, k=5, dil=1),
    "H2L": dict(B=2, T=131, cin=80, cout=1024, k=5, dil=1),      # four column tiles of 256: the lockstep walk of the 256x256 kernel
    "H3": dict(B=5, T=9, cin=128, cout=100, k=3, dil=4),
    "N128": dict(B=3, T=57, cin=36, cout=128, k=3, dil=2),
    "W1032": dict(B=2, T=131, cin=80, cout=1032, k=5, dil=1),
    "W256": dict(B=2, T=131, cin=80, cout=256, k=5, dil=1),
    "W1024": dict(B=2, T=131, cin=80, cout=1024, k=5, dil=1),    # H2L for the wide split form: four column tiles, the lockstep walk
}
# the epilogue of each dense case: (per-segment bias, act, (tee_lo, tee_hi) or None, tee_add)
DENSE = {
    "S1-dense": (True, "relu", (8, 40), True), "S2-dense": (False, "relu", None, False), "S2-dense-tee": (True, None, (128, 256), False),
    "S3-dense": (True, "relu", (4, 52), True), "S4-dense": (False, "relu", None, False),
    "S5-dense": (True, "relu", (8, 40), True), "P-dense": (True, "relu", (8, 40), True),
    "H1-dense": (True, "relu", (8, 40), True), "H2-dense": (False, "relu", None, False), "H2-dense-tee": (True, None, (128, 256), False),
    "H2w-dense-tee": (True, "relu", (128, 256), False), "H3-dense": (True, "relu", (8, 56), True), "H2L-dense": (False, "relu", None, False),
    "N128-split_x": (True, "relu", (0, 128), True), "N128-split_w": (True, None, (0, 128), True),
    "W1032-split_x": (False, "relu", None, False), "W1032-split_w": (False, "relu", (128, 256), False),
    "W256-split_x": (False, "relu", None, False), "W256-split_w": (False, None, None, False), "W1024-split_x": (False, "relu", None, False),
}
GATHER_TEE = {"N128-rows": (0, 128), "H1-rows": (8, 40), "S1-rows": (8, 40), "W1032-rows": (128, 256)}



# ------------------------------------------------------------------ kernels, labels and coverage

F32_CONV_KERNELS = ("conv_gemm_f32_kernel", "conv_gemm_f32_s64_kernel", "skinny_gemm_f32_kernel", "conv_gemm_f32_vh_kernel",
                    "conv_gemm_f32_n64_kernel", "conv_gemm_f32_t256_kernel", "conv_gemm_f32_packed_kernel",
                    "seg_gemm_partial_f32_kernel", "seg_gemm_reduce_f32_kernel")
F16_CONV_KERNELS = ("conv_gemm_f16_kernel", "conv_gemm_f16_t256_kernel")
SPLIT_CONV_KERNELS = ("conv_gemm_split16_n128_kernel", "split16_pack_kernel")
CONV_KERNELS = F32_CONV_KERNELS + F16_CONV_KERNELS + SPLIT_CONV_KERNELS + ("res2net_chain_f16_kernel", "chain_pack_kernel")
REDUCTION_KERNELS = ("seg_mean_std_kernel", "se_scale_residual_kernel", "asp_pool_kernel", "asp_pool_lds_kernel",
                     "asp_attend_pool_f32_kernel", "asp_attend_pool_f16_kernel", "colstat_finish_kernel")
PRODUCT_KERNELS = ("affinity_sym_kernel", "l2norm_rows_kernel", "adjacent_cosine_kernel", "sim_argmax_kernel", "ahc_nearest_kernel",
                   "ahc_nearest_finish_kernel", "ahc_merge_kernel", "affinity_apply_kernel", "apply_finish_kernel",
                   "affinity_degree_kernel", "topk_mean_std_kernel", "viterbi_kernel", "fill_f32_kernel")
ALL_KERNELS = CONV_KERNELS + REDUCTION_KERNELS + PRODUCT_KERNELS


def kernel_of(label):
    """The kernel a launch label names: the text before the first '<' or '/'."""
    return label.replace("/", "<").split("<")[0]


# ---- sd_conv1d_cl_f32: the label of every shape under the eight selections of kernel_selection.CONV_KERNELS.
# sd_choose_conv_f32 (csrc/sd_conv_choice.h), with t128 = ceil(M / 128) ceil(cout / 128), in this order:
#   1. no colstat, T > 1, M >= 64 and t128 < S64 (128; 0 unless "auto"): the 64x64 ring kernel; <32> when ceil(M / 64) ceil(cout / 64) < 128
#   2. no colstat and t128 < SKINNY (128; 0 from "tiles128" on): the 32x32 split-K kernel
#   3. cout >= 1024 and ceil(M / 256) ceil(cout / 256) >= WIDE (1024; 0 under "wide256"), no tee_add, no colstat at T < 128: the 256x256 kernel
#   4. T > 1, and a colstat only for a caller that takes other units (the public entry does not): 80 / 96 / 112 rows when pinned
#      ("auto" / "split32": when 1.02 J / 8 per round of 256 tiles beats 0.97 of the cheaper of 5. and 6.; never on these small shapes)
#   5. 128x64 tiles when pinned ("tiles64"), or by the rule when 0.52 rounds of half tiles < 0.97 rounds of tiles; with a colstat only at
#      T >= 128 and cout % 64 == 0
#   6. the 128x128 kernel, staged by DMA in the shipped build
_S32, _S64 = "conv_gemm_f32_s64_kernel<32>", "conv_gemm_f32_s64_kernel<64>"
_SK, _DMA, _N64, _T256 = "skinny_gemm_f32_kernel", "conv_gemm_f32_kernel<dma>", "conv_gemm_f32_n64_kernel", "conv_gemm_f32_t256_kernel"


def _selections(auto, split32=_SK, tiles64=_N64, rows=True, wide256=_DMA):
    vh = {f"rows{16 * j}": f"conv_gemm_f32_vh_kernel<{j}>" if rows else _DMA for j in (5, 6, 7)}
    return {"auto": auto, "split32": split32, "tiles128": _DMA, "tiles64": tiles64, **vh, "wide256": wide256}


F32_LABELS = {
    "S1": _selections(_S32),                        # t128 = 2; M = 171 >= 64, 3 x 2 tiles of 64x64
    "S2": _selections(_S32, wide256=_T256),         # t128 = 27; 5 x 17 = 85 tiles of 64x64; cout >= 1024: 2 x 5 tiles of 256x256
    "S3": _selections(_SK),                         # M = 45 < 64: rule 1 does not apply, rule 2 does (t128 = 1)
    "S4": _selections(_SK, rows=False),             # T = 1: neither rule 1 nor rule 4
    "S5": _selections(_S64),                        # t128 = 8 x 4 = 32 < 128, 16 x 8 = 128 tiles of 64x64: not < 128
    # with a colstat rules 1, 2 and 4 are out.  (3, 128) x 256: t128 = 6, 12 half tiles, one round each, 0.52 < 0.97 -> rule 5 by itself
    "C3x128-256": _selections(_N64, split32=_N64, rows=False),
    "C5x64-256": _selections(_DMA, split32=_DMA, tiles64=_DMA, rows=False),       # T = 64 < 128: rule 5 is out as well
}
SEG_GEMM_LABELS = ("seg_gemm_partial_f32_kernel", "seg_gemm_reduce_f32_kernel")    # S4 through sd_seg_gemm_f32: M <= 256, cin_pad = 544 >= 512
PACKED_LABEL = "conv_gemm_f32_packed_kernel"

# ---- sd_conv1d_cl_f16: the 128x128 kernel <x, y> unless x is f16, cout >= 1024, the launch is not "small" (cout <= 1024 and at most
# SD_TUNE_F16_NARROW_TILES tiles of 256x256: 128 shipped = "auto", 0 = "wide256"), there is no tee_add and no colstat at T < 128.  Then the
# 256x256 kernel <y, epilogue>: "direct" (registers) for relu / identity with a per-channel bias, no tee and aligned slices, else "staged";
# the direct form walks in lockstep when the column tiles come in fours and there are at least SD_TUNE_T256_LOCKSTEP_TILES tiles
# (shipped: 1024, so never here; the tests pin 0), else one workgroup per tile ("grid").
H_EPILOGUE = {"H2-rows": "direct", "H2-chan": "direct", "H2-dense": "direct", "H2-dense-tee": "staged", "H2w-dense-tee": "staged",
              "H2L-rows": "direct", "H2L-dense": "direct", "C3x128-1024": "direct"}       # the cases with cout >= 1024 that may take it


def _cout(name):
    return SHAPES[name.split("-")[0]]["cout"] if name.split("-")[0] in SHAPES else int(name.split("-")[1])


def f16_label(name, tiles, x16, y16, lockstep=False):
    """The label of one sd_conv1d_cl_f16 run of case `name`: tiles "auto" / "wide256", f16 or f32 x and y, lockstep tuning 0 or shipped."""
    x, y = ("f16" if x16 else "f32"), ("f16" if y16 else "f32")
    cout = _cout(name)
    if not (x16 and name in H_EPILOGUE and (cout > 1024 or tiles == "wide256")):
        return f"conv_gemm_f16_kernel<{x},{y}>"
    walk = "lockstep" if lockstep and H_EPILOGUE[name] == "direct" and -(-cout // 256) % 4 == 0 else "grid"
    return f"conv_gemm_f16_t256_kernel<{y},{H_EPILOGUE[name]}>/{walk}"


# ---- sd_conv1d_cl_split16: f32 x (the narrow form) -> the 128x128 kernel; x packed by sd_split16_pack_f32 -> the 256x256 kernel
# <split, epilogue>, "staged" as well whenever y is written as split halves; walks as above
W_EPILOGUE = {"W1032-rows": "staged", "W1032-split_x": "direct", "W1032-split_w": "staged", "W256-chan": "direct", "W256-split_x": "direct",
              "W256-split_w": "direct", "W1024-chan": "direct", "W1024-split_x": "direct", "C3x128-256": "direct"}


def split_labels(name, split_out=False, lockstep=False):
    """The labels of one sd_conv1d_cl_split16 run (the wide form packs its activations first)."""
    if name[0] == "N":
        return ("conv_gemm_split16_n128_kernel",)
    form = "staged" if split_out else W_EPILOGUE[name]
    walk = "lockstep" if lockstep and form == "direct" and -(-_cout(name) // 256) % 4 == 0 else "grid"
    return ("split16_pack_kernel", f"conv_gemm_f16_t256_kernel<split,{form}>/{walk}")


def _f32(shape, seg=False):
    return tuple(sorted(set(F32_LABELS[shape].values()) | set(SEG_GEMM_LABELS if seg else ())))


def _f16(name, lockstep):
    runs = {f16_label(name, t, x, y) for t in ("auto", "wide256") for x in (True, False) for y in (True, False)}
    if lockstep:
        runs |= {f16_label(name, t, True, y, True) for t in ("auto", "wide256") for y in (True, False)}
    return tuple(sorted(runs))


def _split(name):
    return tuple(sorted(set(split_labels(name)) | set(split_labels(name, split_out=True) if _cout(name) % 32 == 0 else ())
                        | set(split_labels(name, lockstep=True) if _cout(name) == 1024 else ())))


_CS = ("colstat_finish_kernel<f16>", "colstat_finish_kernel<f32>")
_REDUCE = tuple(f"seg_mean_std_kernel<{t},uniform,{f}>" for t in ("f32", "f16") for f in ("16x16", "64x4")) + \
    tuple(f"se_scale_residual_kernel<{t},uniform>" for t in ("f32", "f16"))
_REDUCE_PACKED = tuple(f"{k}<{t},packed{f}>" for k, f in (("seg_mean_std_kernel", ",64x4"), ("se_scale_residual_kernel", "")) for t in ("f32", "f16"))
_POOL = ("asp_pool_lds_kernel<f32>", "asp_pool_lds_kernel<f16>", "asp_pool_kernel<f32,uniform>", "asp_pool_kernel<f16,uniform>")
_POOL_PACKED = ("asp_pool_kernel<f32,packed>", "asp_pool_kernel<f16,packed>")
_FUSED = tuple(f"asp_attend_pool_f32_kernel<{n}{s}>" for n in (4, 8, 13, 16) for s in ("", ",split")) + \
    tuple(f"asp_attend_pool_f16_kernel<{n}>" for n in (1, 2, 3, 4))
_CHAIN = tuple(f"res2net_chain_f16_kernel<{n}>" for n in range(1, 8)) + ("chain_pack_kernel", "conv_gemm_f16_kernel<f16,f16>")
_AFFINITY = ("affinity_sym_kernel<exact f32>", "affinity_sym_kernel<split16x3>", "l2norm_rows_kernel", "adjacent_cosine_kernel")
# the forms of ops.cosine_affinity that are not the triangle kernel: an odd ldo or N % 4 != 0 (f32: the symmetric conv launch, which the
# 32x32 split-K kernel takes below 128 tiles of 128x128 and the 128x128 kernel's band walk from there on; split16: 2^-8 as a per-column
# scale, filled, and every tile through the wide split conv, whose slices are unaligned here: the staged epilogue) and `rows=` blocks
_AFFINITY_CONV = ("skinny_gemm_f32_kernel", "conv_gemm_f32_kernel<dma>/symmetric", "fill_f32_kernel", "split16_pack_kernel",
                  "conv_gemm_f16_t256_kernel<split,staged>/grid")
_AHC = ("ahc_nearest_kernel", "ahc_nearest_finish_kernel", "ahc_merge_kernel")
# sd_affinity_apply_f32: one block of 16 columns per thread up to b = 16, two above; 16-byte loads of K when its rows are 16-byte aligned
_SPECTRAL = tuple(f"affinity_apply_kernel<{nj},{ld}>" for nj in (1, 2) for ld in ("vec", "scalar")) + ("apply_finish_kernel", "affinity_degree_kernel")

# case name -> (kind, labels its runs reach); kind: "gather" (one-hot weights, one-hot logits, planted ties: the answer names the
# element that was read) or "dense" (integer arithmetic over every element)
CASE_TABLE = {
    **{f"{s}-{w}": ("gather", _f32(s, s == "S4")) for s in ("S1", "S2", "S3", "S4", "S5") for w in ("rows", "chan")},
    "S1-dense": ("dense", _f32("S1")), "S2-dense": ("dense", _f32("S2")), "S2-dense-tee": ("dense", _f32("S2")), "S3-dense": ("dense", _f32("S3")),
    "S4-dense": ("dense", _f32("S4", True)), "S5-dense": ("dense", _f32("S5")),
    "P-rows": ("gather", (PACKED_LABEL,)), "P-chan": ("gather", (PACKED_LABEL,)), "P-dense": ("dense", (PACKED_LABEL,)),
    **{f"{s}-{w}": ("gather", _f16(f"{s}-{w}", s == "H2")) for s in ("H1", "H2", "H3") for w in ("rows", "chan")},
    "H1-dense": ("dense", _f16("H1-dense", False)), "H2-dense": ("dense", _f16("H2-dense", True)),
    "H2-dense-tee": ("dense", _f16("H2-dense-tee", True)), "H2w-dense-tee": ("dense", _f16("H2w-dense-tee", True)),
    "H3-dense": ("dense", _f16("H3-dense", False)), "H2L-rows": ("gather", _f16("H2L-rows", True)), "H2L-dense": ("dense", _f16("H2L-dense", True)),
    "N128-rows": ("gather", _split("N128-rows")), "N128-chan": ("gather", _split("N128-chan")),
    "N128-split_x": ("dense", _split("N128-split_x")), "N128-split_w": ("dense", _split("N128-split_w")),
    "W1032-rows": ("gather", _split("W1032-rows")), "W1032-split_x": ("dense", _split("W1032-split_x")), "W1032-split_w": ("dense", _split("W1032-split_w")),
    "W256-chan": ("gather", _split("W256-chan")), "W256-split_x": ("dense", _split("W256-split_x")), "W256-split_w": ("dense", _split("W256-split_w")),
    "W1024-chan": ("gather", _split("W1024-chan")), "W1024-split_x": ("dense", _split("W1024-split_x")),
    "C3x128-256": ("dense", tuple(sorted(set(_f32("C3x128-256")) | set(_f16("C3x128-256", False)) | set(split_labels("C3x128-256")))) + _CS),
    "C5x64-256": ("dense", tuple(sorted(set(_f32("C5x64-256")) | set(_f16("C5x64-256", False)))) + _CS),
    "C11x64-1024": ("dense", _f16("C11x64-1024", False) + _CS), "C3x128-1024": ("dense", _f16("C3x128-1024", False) + _CS),
    "chain-onehot": ("gather", _CHAIN), "chain-sums": ("dense", _CHAIN),
    "reduce-int": ("dense", _REDUCE + _REDUCE_PACKED), "reduce-poison": ("gather", ("seg_mean_std_kernel<f32,uniform,16x16>", "seg_mean_std_kernel<f16,uniform,16x16>")),
    "pool-onehot": ("gather", _POOL + _POOL_PACKED), "pool-uniform": ("dense", _POOL),
    "fused-onehot": ("gather", _FUSED), "fused-uniform": ("dense", _FUSED),
    "affinity-k16": ("dense", _AFFINITY + _AFFINITY_CONV), "affinity-duplicates": ("gather", _AFFINITY),
    "ahc-ties": ("gather", _AHC), "ahc-int": ("dense", _AHC),
    "spectral-dyadic": ("dense", _SPECTRAL), "spectral-onehot": ("gather", _SPECTRAL),
    "argmax-duplicates": ("gather", ("sim_argmax_kernel",)), "argmax-int": ("dense", ("sim_argmax_kernel",)),
    "topk-ties": ("gather", ("topk_mean_std_kernel",)), "topk-int": ("dense", ("topk_mean_std_kernel",)),
    "viterbi-ties": ("gather", ("viterbi_kernel",)), "viterbi-int": ("dense", ("viterbi_kernel",)),
}
assert all(kind in ("gather", "dense") and {kernel_of(lb) for lb in ks} <= set(ALL_KERNELS) for kind, ks in CASE_TABLE.values())


def register(name, kind=None):
    """The kernels of a case; a generator may only build what the table names."""
    if name not in CASE_TABLE:
        raise KeyError(f"{name} is not in CASE_TABLE")
    if kind is not None and CASE_TABLE[name][0] != kind:
        raise ValueError(f"{name} is a {CASE_TABLE[name][0]} case, built as {kind}")
    return CASE_TABLE[name][1]


def coverage(table=None):
    """label -> case names, the inverse of CASE_TABLE."""
    out = {}
    for name, (_, kernels) in (CASE_TABLE if table is None else table).items():
        for k in kernels:
            out.setdefault(k, []).append(name)
    return out


EXACT_COVERAGE = coverage()


# ------------------------------------------------------------------ convs

def source_rows(lengths, k, dil):
    """[M, k] int64: the row tap j of output row m reads, reflected inside m's segment (segments given by their lengths)."""
    src = []
    start = 0
    for L in lengths:
        if (k // 2) * dil >= L:
            raise ValueError(f"reflect padding {(k // 2) * dil} needs a longer segment than {L}")
        t = np.arange(L)[:, None] + (np.arange(k)[None, :] - k // 2) * dil
        t = np.where(t < 0, -t, t)
        t = np.where(t >= L, 2 * (L - 1) - t, t)
        src.append(start + t)
        start += L
    return np.concatenate(src).astype(np.int64)


def conv_sum(x, w, src):
    """sum_j x[src[:, j]] @ w[:, :, j].T in float64 (exact: every partial sum is an integer multiple of a power of two far below 2^53)."""
    acc = np.zeros((x.shape[0], w.shape[0]), dtype=np.float64)
    for j in range(w.shape[2]):
        acc += x[src[:, j]].astype(np.float64) @ w[:, :, j].astype(np.float64).T
    return acc


@dataclass
class ConvCase:
    name: str
    kind: str                   # "rows" / "chan" (gather), "dense", "split_x" / "split_w" (the 2049 s operand on that side)
    lengths: tuple              # segment lengths: (T,) * B, or the packed spans
    packed: bool
    cin: int
    cout: int
    k: int
    dil: int
    x: np.ndarray               # [M, cin] float64 (integers)
    w: np.ndarray               # [cout, cin, k] float64
    bias: np.ndarray = None     # [cout] or [B, cout]
    bias_per_seg: bool = False
    act: str = None
    scale: np.ndarray = None
    shift: np.ndarray = None
    tee_lo: int = 0
    tee_hi: int = 0             # 0: no tee
    tee_add: np.ndarray = None  # [M, tee_hi - tee_lo]
    y: np.ndarray = None        # expected [M, cout] float64
    tee: np.ndarray = None      # expected [M, tee_hi - tee_lo]
    kernels: tuple = ()
    bound: float = 0.0          # sum |x| |w| of the largest output: no partial sum, in any order, passes it
    f16: bool = False           # the case is also run with f16 storage
    e: int = 0                  # a twin: the value operands (x, bias, shift, tee_add; "w:-q": w instead of x) times 2^e

    @property
    def M(self):
        return int(sum(self.lengths))

    @property
    def B(self):
        return len(self.lengths)

    @property
    def T(self):
        return self.lengths[0]

    @property
    def frame_start(self):
        return np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int32)


def conv_epilogue(c: ConvCase, acc):
    """bias, relu, scale, shift and the tee of case `c` on the accumulators `acc`, in float64: sets c.y / c.tee, returns every
    intermediate an f32 epilogue holds."""
    r = acc
    steps = [acc]
    if c.bias is not None:
        r = r + (np.repeat(c.bias, c.lengths, axis=0) if c.bias_per_seg else c.bias[None, :])
        steps.append(r)
    if c.act == "relu":
        r = np.maximum(r, 0.0)
    if c.scale is not None:
        r = r * c.scale[None, :]
        steps.append(r)
    if c.shift is not None:
        r = r + c.shift[None, :]
        steps.append(r)
    c.y = r
    if c.tee_hi:
        c.tee = r[:, c.tee_lo:c.tee_hi] + (c.tee_add if c.tee_add is not None else 0.0)
        steps.append(c.tee)
    return steps


def conv_twin(c: ConvCase, e, storage, side="x") -> ConvCase:
    """Case `c` with its value operands times 2^e: x (side "w": the weights instead, for the split operator, whose host pack absorbs
    the factor into its 2^s), bias, shift and tee_add; scale stays.  Every operation of the operator is homogeneous of degree one in
    them, so the expected y and tee are ldexp(., e) -- unless the split operator cannot carry x 2^e in two f16 halves (2049 2^-26),
    where they are what `split16_conv_sum` makes of the halves.  `storage`: "f32", "f16" (x, y, tee, tee_add stored as f16) or
    "split" (x carried as f16 halves, y f32).  The budget is checked on the scaled values."""
    t = ConvCase(**{**c.__dict__, "e": e, "name": f"{c.name}@{side if side != 'x' else ''}2^{e}"})
    if side == "x":
        t.x = scaled(e, c.x)
    else:
        t.w = scaled(e, c.w)
    t.bias, t.shift, t.tee_add = scaled(e, c.bias, c.shift, c.tee_add)
    src = source_rows(c.lengths, c.k, c.dil)
    if np.ldexp(c.bound, e) >= 2.0 ** 127:
        raise BudgetError(f"{t.name}: sum |x| |w| reaches 2^127")
    acc = split16_conv_sum(t.x, t.w, src) if storage == "split" else conv_sum(t.x, t.w, src)
    steps = conv_epilogue(t, acc)
    need_f32(t.name, *steps, *([t.tee_add] if t.tee_add is not None else []), e=e)
    need_f32(t.name, t.x if side == "x" else t.w, e=e)
    if storage == "f16":
        need_f16(t.name, t.x, t.y, *([t.tee] if t.tee_hi else []), *([t.tee_add] if t.tee_add is not None else []), e=e)
    return t


def finish_conv(c: ConvCase) -> ConvCase:
    """Fill in the expected outputs and check the budget for every storage type the case is run with."""
    src = source_rows(c.lengths, c.k, c.dil)
    acc = conv_sum(c.x, c.w, src)
    c.bound = float(conv_sum(np.abs(c.x), np.abs(c.w), src).max())
    if c.bound >= F32_LIMIT:
        raise BudgetError(f"{c.name}: sum |x| |w| = {c.bound:g} reaches 2^24")
    steps = conv_epilogue(c, acc)
    need_f32(c.name, *steps, c.x, c.w)
    if c.f16:
        need_f16(c.name, c.x, c.w, c.y, *([c.tee] if c.tee_hi else []), *([c.tee_add] if c.tee_add is not None else []))
    return c


def _lengths(s):
    return tuple(s["spans"]) if "spans" in s else (s["T"],) * s["B"]


def gather_case(name, s, which, *, f16=False, seed=0, tee=None):
    """One-hot weights: w[n][jmap(n)][cmap(n)] = 1.  x[m, c] = m ("rows") makes y[m, n] the reflected source row of tap jmap(n),
    x[m, c] = c ("chan") makes it the source channel cmap(n); both maps are seeded and use every tap and the channels 0 and cin - 1
    (the last real one before the cin_pad zero fill)."""
    cin, cout, k = s["cin"], s["cout"], s["k"]
    rng = np.random.default_rng(seed + 17 * cout + cin)
    lengths = _lengths(s)
    M = sum(lengths)
    cmap = np.concatenate([rng.permutation(cin) for _ in range(-(-cout // cin))])[:cout]
    cmap[:2] = (cin - 1, 0)
    jmap = rng.permutation(cout) % k
    w = np.zeros((cout, cin, k))
    w[np.arange(cout), cmap, jmap] = 1.0
    x = np.repeat(np.arange(M, dtype=np.float64)[:, None], cin, 1) if which == "rows" else np.repeat(np.arange(cin, dtype=np.float64)[None, :], M, 0)
    c = ConvCase(name, which, lengths, "spans" in s, cin, cout, k, s["dil"], x, w, kernels=register(name, "gather"), f16=f16)
    if tee:
        c.tee_lo, c.tee_hi = tee
    c = finish_conv(c)
    want = source_rows(lengths, k, s["dil"])[:, jmap] if which == "rows" else np.repeat(cmap[None, :], M, 0)
    assert np.array_equal(c.y, want.astype(np.float64)), name          # the conv IS the gather
    return c


def dense_case(name, s, *, f16=False, seed=0, bias_per_seg=False, act="relu", tee=None, tee_add=False, kind="dense", kernels=None):
    """x, w in {-2 .. 2}; integer bias (per channel or per segment); scale in {0.5, 1, 2, 4}; integer shift; relu or identity; a partial
    tee [tee_lo, tee_hi) with an integer tee_add.  kind "split_x" / "split_w": that operand is 2049 s, s in {-1, 0, 1}
    (f16(2049) = 2048, remainder 1: hi and lo both carry weight; the other operand has no low half, so lo.lo is zero)."""
    cin, cout, k = s["cin"], s["cout"], s["k"]
    rng = np.random.default_rng(seed + 31 * cout + cin)
    lengths = _lengths(s)
    M, B = sum(lengths), len(lengths)
    x = rng.integers(-2, 3, (M, cin)).astype(np.float64)
    w = rng.integers(-2, 3, (cout, cin, k)).astype(np.float64)
    if kind == "split_x":
        x = 2049.0 * rng.integers(-1, 2, (M, cin))
    if kind == "split_w":
        w = 2049.0 * rng.integers(-1, 2, (cout, cin, k))
    big = 1 if kind == "dense" else 2049
    bias = big * rng.integers(-8, 9, (B, cout) if bias_per_seg else (cout,)).astype(np.float64)
    c = ConvCase(name, kind, lengths, "spans" in s, cin, cout, k, s["dil"], x, w, bias=bias, bias_per_seg=bias_per_seg, act=act,
                 scale=rng.choice(np.array([0.5, 1.0, 2.0, 4.0]), cout), shift=rng.integers(-9, 10, cout).astype(np.float64),
                 kernels=register(name, "dense") if kernels is None else kernels, f16=f16)
    if tee:
        c.tee_lo, c.tee_hi = tee
        if tee_add:
            c.tee_add = rng.integers(-5, 6, (M, tee[1] - tee[0])).astype(np.float64)
    return finish_conv(c)


def oversized_case():
    """A 2049 s case whose accumulator bound passes 2^24: the helper must refuse it (BudgetError)."""
    return dense_case("oversized", dict(B=1, T=8, cin=32768, cout=8, k=1, dil=1), kind="split_x", kernels=())


def colstat_case(name, B, T, cout, seed=0):
    """1x1 conv, cin 64, relu + affine with y - shift in {0 .. 3} and T a power of two.  Columns n % 3 == 0: half the rows 0 and half 2
    (variance exactly 1); n % 3 == 1: constant (variance 0 -> sqrt(eps)); n % 3 == 2: a pattern over {0 .. 3} that depends on the frame
    and the segment (exact mean; the std only where the variance is a perfect square)."""
    if T & (T - 1):
        raise BudgetError(f"{name}: T = {T} is no power of two")
    rng = np.random.default_rng(seed + cout + T)
    cin, M = 64, B * T
    t, b = np.arange(M) % T, np.arange(M) // T
    x = rng.integers(-2, 3, (M, cin)).astype(np.float64)          # channels 10 .. 63 meet zero weights
    x[:, :10] = 0.0
    x[np.arange(M), (t * 5 + b) % 8] = 1.0
    x[:, 8] = t % 2
    x[:, 9] = 1.0
    w = np.zeros((cout, cin, 1))
    n = np.arange(cout)
    w[n % 3 == 0, 8, 0] = 2.0
    w[n % 3 == 1, 9, 0] = rng.integers(0, 4, (n % 3 == 1).sum())
    w[n % 3 == 2, :8, 0] = rng.integers(0, 5, ((n % 3 == 2).sum(), 8))
    c = ConvCase(name, "dense", (T,) * B, False, cin, cout, 1, 1, x, w, bias=np.where(n % 3 == 2, -1.0, 0.0), act="relu", scale=np.ones(cout),
                 shift=rng.integers(-3, 4, cout).astype(np.float64), kernels=register(name, "dense"), f16=True)
    c = finish_conv(c)
    v = c.y - c.shift[None, :]
    if v.min() < 0 or v.max() > 3:
        raise BudgetError(f"{name}: y - shift leaves {{0 .. 3}}")
    need_mean(name, v.reshape(B, T, cout).sum(1), T)
    return c


def colstat_units(c: ConvCase, unit=128):
    """[units, 6, cout] float64: per tile of `unit` rows [sum part 0..2 | sum of squares part 0..2] of y - shift, a part being the
    tile's first, second or third segment; NaN where a part has no rows (a kernel may leave such a slot alone)."""
    v = c.y - c.shift[None, :]
    M, T = c.M, c.T
    units = -(-M // unit)
    out = np.full((units, 6, c.cout), np.nan)
    for u in range(units):
        rows = np.arange(u * unit, min(M, (u + 1) * unit))
        part = rows // T - (u * unit) // T
        for p in range(3):
            sel = rows[part == p]
            if sel.size:
                out[u, p] = v[sel].sum(0)
                out[u, 3 + p] = (v[sel] ** 2).sum(0)
    need_f32(c.name + " (colstat)", np.nan_to_num(out[:, :3]), e=c.e)
    need_f32(c.name + " (colstat)", np.nan_to_num(out[:, 3:]), e=2 * c.e)
    return out


SQRT_EPS = float(np.sqrt(np.float32(1e-12)))      # what sqrtf(fmaxf(0, 1e-12f)) returns: 1e-6 to f32 rounding


def twin_eps(e=0):
    """f32(1e-12) 4^e: the variance clamp of a twin at 2^e, a normal f32 for every exponent used here."""
    eps = float(np.float32(1e-12)) * 4.0 ** e
    if not 2.0 ** -126 <= eps < 2.0 ** 128 or float(np.float32(eps)) != eps:
        raise BudgetError(f"eps 4^{e} = {eps:g} is no normal f32")
    return eps


def exact_std(var):
    """sqrt(var) where the variance is the square of a dyadic number, SQRT_EPS where it is 0, NaN (= not asserted) elsewhere."""
    var = np.asarray(var, dtype=np.float64)
    root = np.sqrt(var)
    return np.where(var == 0, SQRT_EPS, np.where(root * 64 == np.round(root * 64), root, np.nan))


def colstat_stats(c: ConvCase):
    """(mean, std) per segment; of a twin: ldexp of the unscaled statistics (sqrt(eps 4^e) = sqrt(eps) 2^e where the variance is 0)."""
    yr = np.ldexp(c.y, -c.e).reshape(c.B, c.T, c.cout)
    return scaled(c.e, yr.mean(1), exact_std(yr.var(1)))


def default_storage(name):
    """How the operator a case is built for carries its activations: H* as f16, N* / W* as two f16 halves, the others as f32."""
    return {"H": "f16", "N": "split", "W": "split"}.get(name[0], "f32")


@functools.lru_cache(maxsize=None)
def _conv_twin(name, e, storage, side):
    return conv_twin(_conv_case(name), e, storage, side)


def conv_case(name, e=0, storage=None, side="x"):
    """Every conv case of CASE_TABLE by name (built once per process, never modified).  `e` != 0: its twin at 2^e (`conv_twin`) for the
    storage given (default: that of the operator the case is named for)."""
    return _conv_twin(name, e, storage or default_storage(name), side) if e else _conv_case(name)


@functools.lru_cache(maxsize=None)
def _conv_case(name):
    shape, _, what = name.partition("-")
    if shape[0] == "C":
        bt, cout = name[1:].split("-")
        B, T = (int(v) for v in bt.split("x"))
        return colstat_case(name, B, T, int(cout))
    s = SHAPES[shape]
    f16 = shape[0] == "H"
    if what in ("rows", "chan"):
        return gather_case(name, s, what, f16=f16, tee=GATHER_TEE.get(name))
    per_seg, act, tee, add = DENSE[name]
    kind = what if what.startswith("split") else "dense"
    return dense_case(name, s, f16=f16, bias_per_seg=per_seg, act=act, tee=tee, tee_add=add, kind=kind)


CONV_CASE_NAMES = tuple(n for n in CASE_TABLE if n.split("-")[0] in SHAPES or n[0] == "C" and n[1].isdigit())


# ------------------------------------------------------------------ the Res2Net chain

# (B, T, dil): one instantiation of the chain kernel per 32-row time tile, ceil(T / 32) = 1 .. 7 -- T = 32 the upper edge of the first,
# 65 / 97 / 129 / 161 the first T of the third to sixth, 61 and 212 (the longest the kernel takes) the second and the seventh
CHAIN_SHAPES = ((3, 61, 3), (2, 212, 4), (2, 32, 2), (2, 65, 3), (2, 97, 2), (2, 129, 3), (2, 161, 4))


@functools.lru_cache(maxsize=None)
def chain_case(kind, B, T, dil, n=7, ld=1024 + 64, e=0):
    """"onehot": one-hot weights [128][128][3], so the chain is a composition of gathers and adds; "sums": four +-1 weights per output
    channel (taps and channels mixed), so every output is a signed sum.  Integer bias / shift, scale 1 (layer 3: 2), relu.
    -> (r [B T, ld] small integers, layers, the expected r after the chain); every chain state y_j and c_{j+1} + y_j an exact f16.
    `e`: the twin with r, every bias and every shift times 2^e, whose chain is ldexp(., e) state by state."""
    name = "chain-" + kind
    register(name, "gather" if kind == "onehot" else "dense")
    rng = np.random.default_rng(T + dil + (kind == "sums"))
    M = B * T
    r = rng.integers(0, 3, (M, ld)).astype(np.float64)
    src = source_rows((T,) * B, 3, dil)
    layers = []
    states = []
    out = r.copy()
    u = r[:, 128:256].copy()
    for j in range(1, n + 1):
        w = np.zeros((128, 128, 3))
        if kind == "onehot":
            w[np.arange(128), rng.permutation(128), rng.permutation(128) % 3] = 1.0
        else:
            for q in range(4):
                w[np.arange(128), rng.permutation(128), (rng.permutation(128) + q) % 3] += rng.choice(np.array([-1.0, 1.0]), 128)
        L = dict(w=w, bias=rng.integers(-2, 2, 128).astype(np.float64), scale=np.full(128, 2.0 if j == 3 else 1.0),
                 shift=rng.integers(-1, 3, 128).astype(np.float64), dil=dil)
        acc = conv_sum(u, w, src)
        y = np.maximum(acc + L["bias"][None, :], 0.0) * L["scale"][None, :] + L["shift"][None, :]
        need_f32(name, conv_sum(np.abs(u), np.abs(w), src))
        need_f16(name, y, u)
        states += [y, u]
        out[:, 128 * j:128 * j + 128] = y
        if j < n:
            u = y + r[:, 128 * (j + 1):128 * (j + 2)]
        layers.append(L)
    if e:
        need_f16(name, *scaled(e, r, *states), e=e)
        need_f32(name, *scaled(e, *states), e=e)
        r, out = scaled(e, r, out)
        layers = [dict(L, bias=scaled(e, L["bias"]), shift=scaled(e, L["shift"])) for L in layers]
    return r, layers, out


# ------------------------------------------------------------------ reductions

LENS = ((201, 128), (131, 64), (57, 32))        # (T, n): rel_len = f32(n / T) gives mask_frames = norm_frames = n
POISON = 1e30
POISON_F16 = 65504.0


def rel_len(T, n):
    return np.float32(n / T)


def reduction_case(B, T, C, lens=None, f16=False, seed=0, e=0):
    """The case below (built once per process, never modified), or its twin at 2^e: x and res times 2^e (the gate and the poison stay)
    and `eps` = f32(1e-12) 4^e; mean, std and y are ldexp(., e), and the std of a constant column sqrt(eps) 2^e."""
    d = _reduction_case(B, T, C, lens, f16, seed)
    if not e:
        return d
    name = "reduce-poison" if lens else "reduce-int"
    x, res, mean, std, y = scaled(e, d["x"], d["res"], d["mean"], d["std"], d["y"])
    need_f32(name, x, res, mean, y, e=e)
    need_f32(name, scaled(2 * e, d["sq"]), e=2 * e)
    if f16:
        need_f16(name, x, res, y, e=e)
    xp = np.where(np.arange(T)[None, :, None] < d["n_live"][:, None, None], x, d["x_poisoned"])
    return dict(d, x=x, x_poisoned=xp, res=res, mean=mean, std=std, y=y, eps=twin_eps(e))


@functools.lru_cache(maxsize=None)
def _reduction_case(B, T, C, lens, f16, seed):
    """Integer x [B, T, C] in {-3 .. 3} (columns 0 mod 5: 0 / 2 alternating, variance 1 over an even number of frames; 1 mod 5: constant),
    gate in {0.25, 0.5, 1}, integer res.  `lens`: the live frames of each segment in turn; the frames past them hold POISON (f16: the
    largest f16) in `x_poisoned`.  -> dict with the expected mean / std (NaN where the variance is no perfect square) over the live
    frames and y = x gate + res over all rows (`sq`: the sums of squared deviations, for the twins' budget)."""
    name = "reduce-poison" if lens else "reduce-int"
    register(name)
    rng = np.random.default_rng(seed + C + T)
    n_live = np.array([lens[b % len(lens)] for b in range(B)]) if lens else np.full(B, T)
    x = rng.integers(-3, 4, (B, T, C)).astype(np.float64)
    x[:, :, 0::5] = np.where(np.arange(T)[None, :, None] % 2, 2.0, 0.0)
    x[:, :, 1::5] = rng.integers(-3, 4, (B, 1, len(range(1, C, 5))))
    gate = rng.choice(np.array([0.25, 0.5, 1.0]), (B, C))
    res = rng.integers(-4, 5, (B, T, C)).astype(np.float64)
    mean, std = np.zeros((B, C)), np.zeros((B, C))
    for b in range(B):
        live = x[b, :n_live[b]]
        need_mean(name, live.sum(0), int(n_live[b]))
        mean[b] = live.mean(0)
        need_f32(name, ((live - mean[b]) ** 2).sum(0))
        std[b] = exact_std(live.var(0))
    y = x * gate[:, None, :] + res
    need_f32(name, y)
    if f16:
        need_f16(name, x, res, y)
    xp = x.copy()
    for b in range(B):
        xp[b, n_live[b]:] = POISON_F16 if f16 else POISON
    sq = np.stack([((x[b, :n_live[b]] - mean[b]) ** 2).sum(0) for b in range(B)])
    return dict(x=x, x_poisoned=xp, gate=gate, res=res, mean=mean, std=std, y=y, n_live=n_live, eps=twin_eps(0), sq=sq)


def pool_frames(T):
    """Frames on both sides of every boundary of the pooling kernels: the 4 row phases of the streaming kernel, the 8 (f32) / 4 (f16) row
    phases and the 32-row staging passes of the LDS kernel, the 16-frame MFMA tiles, the 64-frame wave slots and the 64 / 128 / 192 /
    208-frame templates of the fused kernels; the first and the last frame."""
    cand = [0, 1, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 207, 208, 209, 247, 248, T - 2, T - 1]
    return sorted({t for t in cand if 0 <= t < T})


@functools.lru_cache(maxsize=None)
def pool_onehot_case(B, T, C, lens=None, fused=False, seed=0, e=0, f16=False):
    """logit 0 at frame t*(b, c) and -200 elsewhere (exp underflows to exactly 0; -200 is an f16 value), integer h: the mean is
    h[b, t*, c] and the variance 0.  t* walks pool_frames() below the live frames.  Padded frames hold a +200 logit and POISON in h
    (`h_f16`: the largest f16)."""
    name = "fused-onehot" if fused else "pool-onehot"
    register(name, "gather")
    rng = np.random.default_rng(seed + T + C)
    n_live = np.array([lens[b % len(lens)] for b in range(B)]) if lens else np.full(B, T)
    h = rng.integers(-9, 10, (B, T, C)).astype(np.float64)
    logit = np.full((B, T, C), -200.0)
    tstar = np.zeros((B, C), dtype=np.int64)
    for b in range(B):
        fr = np.array(pool_frames(int(n_live[b])))
        tstar[b] = fr[(np.arange(C) // (4 if fused else 1) + 3 * b) % len(fr)]
        logit[b, tstar[b], np.arange(C)] = 0.0
        logit[b, n_live[b]:] = 200.0
    mean = np.take_along_axis(h, tstar[:, None, :], 1)[:, 0]
    need_f16(name, h, logit)
    hp, hp16 = h.copy(), h.copy()
    for b in range(B):
        hp[b, n_live[b]:] = POISON
        hp16[b, n_live[b]:] = POISON_F16
    if e:                                                   # the twin: h times 2^e (`f16`: stored as f16), the logits and the poison as they are
        (need_f16 if f16 else need_f32)(name, scaled(e, h), e=e)
        live = np.arange(T)[None, :, None] < n_live[:, None, None]
        hp, hp16, mean = np.where(live, scaled(e, h), hp), np.where(live, scaled(e, h), hp16), scaled(e, mean)
    return dict(logit=logit, h=hp, h_f16=hp16, mean=mean, tstar=tstar, n_live=n_live, eps=twin_eps(e), sqrt_eps=np.ldexp(SQRT_EPS, e))


@functools.lru_cache(maxsize=None)
def pool_uniform_case(B, T, C, level=1.0, fused=False, n=None, seed=0, e=0, f16=False):
    """All logits of a channel equal (`level` times a per-channel integer) over the n live frames (all T when n is None), n a power of
    two, integer h: the exact mean, and the exact std on the columns built for it (0 / 2 alternating: variance 1; constant: sqrt(eps)).
    Padded frames hold a +200 logit and POISON in h (`h_f16`: the largest f16)."""
    name = "fused-uniform" if fused else "pool-uniform"
    register(name, "dense")
    n = T if n is None else n
    if n & (n - 1) or n > T:
        raise BudgetError(f"{name}: {n} live frames of {T} are no power of two")
    rng = np.random.default_rng(seed + T + C)
    h = rng.integers(-9, 10, (B, T, C)).astype(np.float64)
    h[:, :, 0::3] = np.where(np.arange(T)[None, :, None] % 2, 2.0, 0.0)
    h[:, :, 1::3] = rng.integers(-9, 10, (B, 1, len(range(1, C, 3))))
    logit = np.repeat(level * rng.integers(-3, 4, (B, 1, C)).astype(np.float64), T, 1) + 0.0
    logit[:, n:] = 200.0
    live = h[:, :n]
    need_mean(name, live.sum(1), n)
    mean = live.mean(1)
    need_f32(name, ((live - mean[:, None]) ** 2).sum(1))
    need_f16(name, h, logit)
    hp, hp16 = h.copy(), h.copy()
    hp[:, n:], hp16[:, n:] = POISON, POISON_F16
    std = exact_std(live.var(1))
    if e:
        (need_f16 if f16 else need_f32)(name, scaled(e, h), e=e)
        need_f32(name, scaled(e, mean), e=e)
        need_f32(name, scaled(2 * e, ((live - mean[:, None]) ** 2).sum(1)), e=2 * e)
        hp[:, :n] = hp16[:, :n] = scaled(e, live)
        mean, std = scaled(e, mean, std)
    return dict(logit=logit, h=hp, h_f16=hp16, mean=mean, std=std, n_live=np.full(B, n), eps=twin_eps(e))


def attend_factors(logit, att=128):
    """One-hot a1 [B, T, att] and integer wc [C, att] with a1 @ wc.T == logit: one attention channel per distinct logit row (the frames
    that are nobody's t* share one, the padded frames another, every t* class has its own)."""
    B, T, C = logit.shape
    rows, inv = np.unique(logit.reshape(B * T, C), axis=0, return_inverse=True)
    if len(rows) > att:
        raise BudgetError(f"{len(rows)} distinct logit rows do not fit {att} attention channels")
    a1 = np.zeros((B * T, att))
    a1[np.arange(B * T), np.asarray(inv).reshape(-1)] = 1.0
    wc = np.zeros((C, att))
    wc[:, :len(rows)] = rows.T
    assert np.array_equal((a1 @ wc.T).reshape(B, T, C), logit)
    return a1.reshape(B, T, att), wc


FUSED_WS = 256.0        # the power of two the public entry of the fused pooling multiplies its weights with before it splits them


def fused_split_logits(a1, wc, flush=False):
    """The logits of the fused pooling's split product in numpy: a1 and wc 2^8 split into f16 halves, hi.hi + hi.lo + lo.hi in float64,
    times 2^-8.  `flush`: what an implementation that dropped f16 subnormals would compute instead."""
    ah, al = split16_halves(a1)
    wh, wl = split16_halves(wc, FUSED_WS)
    if flush:
        ah, al, wh, wl = (np.where(np.abs(v) < 2.0 ** -14, 0.0, v) for v in (ah, al, wh, wl))
    return (ah @ wh.T + ah @ wl.T + al @ wh.T) / FUSED_WS


@functools.lru_cache(maxsize=None)
def fused_split_case(B, T, C, n, side, att=128):
    """The fused pooling's split logits decided by an f16-subnormal low half.  h, mean and std are those of `pool_uniform_case` (n live
    frames, logits 0).  The even live frames get their logit 0 from a zero weight; the odd ones from a sum that cancels only if the
    subnormal takes part:
      side "a1": a1 = (2^-3 + 2^-16, 1) against wc = (1, -(2^-3 + 2^-16)): the halves of 2^-3 + 2^-16 are (2^-3, 2^-16), the low one an
                 f16 subnormal; those of wc 2^8 are (256, 0) and (-32, -2^-8): 32 + 2^-8 - 32 - 2^-8 = 0
      side "wc": a1 = (2^10, 1) against wc = (2049 2^-28, -(2 + 2^-10) 2^-8): the halves of 2049 2^-20 are (2^-9, 2^-20), those of
                 -(2 + 2^-10) are (-2, -2^-10): 2 + 2^-10 - 2 - 2^-10 = 0
    Every partial sum is a small multiple of a power of two, so the accumulators are exactly 0 in any order, the softmax is uniform
    and the answer is the exact mean and std.  Without the subnormal the odd frames sit 2^-16 (2^-18) below the even ones, their
    weights 1.5e-5 (3.8e-6) lower, and the mean of a column that alternates 0 / 2 moves by tens of ulps.  Padded frames: a logit of
    +200 from a channel of their own and POISON in h.  -> dict(a1 [B, T, att], wc [C, att], h, mean, std, n_live, eps)"""
    d = pool_uniform_case(B, T, C, level=0.0, fused=True, n=n)
    pair = {"a1": ((0.125 + 2.0 ** -16, 1.0), (1.0, -(0.125 + 2.0 ** -16))),
            "wc": ((1024.0, 1.0), (2049.0 * 2.0 ** -28, -(2.0 + 2.0 ** -10) / FUSED_WS))}[side]
    a1 = np.zeros((B, T, att))
    a1[:, 1:n:2, 0], a1[:, 1:n:2, 1] = pair[0]
    a1[:, 0:n:2, 2] = 1.0
    a1[:, n:, 3] = 1.0
    wc = np.zeros((C, att))
    wc[:, 0], wc[:, 1] = pair[1]
    wc[:, 3] = 200.0
    need_f32("fused-split", a1, wc)
    logit = fused_split_logits(a1.reshape(B * T, att), wc).reshape(B, T, C)
    if logit[:, :n].any() or not (logit[:, n:] == 200.0).all():
        raise BudgetError(f"fused-split {side}: the live logits are not all 0")
    return dict(d, a1=a1, wc=wc)


# ------------------------------------------------------------------ products outside the network

def affinity_rows(n, d=192, seed=0, e=0):
    """Rows in {0, +-1} with exactly 16 non-zeros (norm 4, cosine k / 16); row 2 zero; rows 1 and n - 1 copies of row 0 (cosine 1).
    -> (X, K) with K[i][j] = k / 16."""
    register("affinity-k16", "dense"), register("affinity-duplicates", "gather")
    rng = np.random.default_rng(seed + n)
    X = np.zeros((n, d))
    for i in range(n):
        X[i, rng.choice(d, 16, replace=False)] = rng.choice(np.array([-1.0, 1.0]), 16)
    X[2] = 0.0
    X[1] = X[0]
    X[n - 1] = X[0]
    K = (X @ X.T) / 16.0
    need_f32("affinity", K * 16.0, K)
    if e:                                                   # the twin: every row times 2^e; the cosines are those of the unscaled rows
        need_f32("affinity", scaled(e, X), e=e)
        need_f32("affinity", scaled(2 * e, np.abs(X) @ np.abs(X).T), e=2 * e)
        X = scaled(e, X)
    return X, K


def ahc_case(n, d, ld, seed=0):
    """Integer cluster sums in {-1, 0, 1} drawn from sixteen distinct rows (NaN in columns [d, ld)), inv_count in {1, 1/2, 1/4, 1/8}:
    nearly every row has many equal best scores.  Planted: copies of one heavy row at indices 16, 64 and 128 apart, on both sides of the diagonal and in the last row,
    with equal counts, so that their mutual score is each one's maximum and every step of the reduction (in-lane, the 16-lane row, the
    two waves through LDS, the slot order of the finish kernel) breaks a tie; three adjacent copies of a second heavy row tie across
    the lanes of a row.  -> (S, count, inv, nn, best), nn the LOWEST index attaining the integer maximum."""
    register("ahc-ties", "gather"), register("ahc-int", "dense")
    rng = np.random.default_rng(seed + n + d)
    S = np.full((n, ld), np.nan)
    S[:, :d] = rng.integers(-1, 2, (16, d))[rng.integers(0, 16, n)]          # sixteen distinct rows, each many times
    count = rng.choice(np.array([1.0, 2.0, 4.0, 8.0]), n)
    heavy = rng.choice(np.array([-3.0, 3.0]), d)
    group = [i for i in (5, 21, 69, 133, 197, 261) if i < n - 1] + [n - 1]
    for i in group:
        S[i, :d] = heavy
        count[i] = 1.0
    second = rng.choice(np.array([-3.0, 3.0]), d)
    second[: d // 2] = -heavy[: d // 2]                     # far from the first group
    for i in (70, 71, 72):
        S[i, :d] = second
        count[i] = 2.0
    inv = 1.0 / count
    G = S[:, :d] @ S[:, :d].T
    score = G * (inv[:, None] * inv[None, :])
    need_f32("ahc", np.abs(S[:, :d]) @ np.abs(S[:, :d]).T, score)
    np.fill_diagonal(score, -np.inf)
    nn = score.argmax(1)                                     # numpy: the first maximum
    best = score[np.arange(n), nn]
    assert all(nn[i] == (group[0] if i != group[0] else group[1]) for i in group) and nn[71] == 70 and nn[70] == 71 and nn[72] == 70
    return S, count, inv, nn.astype(np.int32), best


def spectral_case(n, b, ld, onehot=False, seed=0):
    """K [n, ld] (NaN past column n) with values in {-1, -0.5, 0, 0.25, 0.5, 1}, scale in {0.5, 1, 2}, integer V [n, b]; `onehot`: column c
    of V is one-hot at a seeded row j_c (the first at row 0, the last at row n - 1), so Y[i][c] names the entry K[i][j_c] that was read."""
    register("spectral-onehot" if onehot else "spectral-dyadic")
    rng = np.random.default_rng(seed + n + b)
    K = np.full((n, ld), np.nan)
    K[:, :n] = rng.choice(np.array([-1.0, -0.5, 0.0, 0.25, 0.5, 1.0]), (n, n))
    scale = rng.choice(np.array([0.5, 1.0, 2.0]), n)
    V = rng.integers(-3, 4, (n, b)).astype(np.float64)
    if onehot:
        V[:] = 0.0
        js = rng.integers(0, n, b)
        js[0], js[-1] = 0, n - 1
        V[js, np.arange(b)] = 1.0
    A = np.clip(K[:, :n], 0.0, None)
    need_f32("spectral", A.sum(1), (A * scale[None, :]) @ np.abs(V) * scale[:, None])
    return K, scale, V


def spectral_expected(K, scale, V, zero_diag):
    n = K.shape[0]
    A = np.clip(K[:, :n], 0.0, None)
    if zero_diag:
        A = A.copy()
        np.fill_diagonal(A, 0.0)
    return A.sum(1), scale[:, None] * (A @ (scale[:, None] * V))


def argmax_case(N, K, D, seed=0, e=0):
    """Integer rows and centres, the centres at (0, K - 1) and (3, 4) duplicated: np.argmax returns the first maximum."""
    register("argmax-duplicates", "gather"), register("argmax-int", "dense")
    rng = np.random.default_rng(seed + N + K + D)
    w = rng.integers(-2, 3, (N, D)).astype(np.float64)
    c = rng.integers(-2, 3, (K, D)).astype(np.float64)
    if K > 4:
        c[4] = c[3]
    if K > 1:
        c[K - 1] = c[0]
    if K == 5:
        c[3] = c[0]                                         # (K - 1 == 4: the two pairs share a centre)
    sim = w @ c.T
    need_f32("sim_argmax", np.abs(w) @ np.abs(c).T)
    if e:                                                   # the twin: the rows times 2^e -- the same index, the score times 2^e
        need_f32("sim_argmax", scaled(e, w), scaled(e, np.abs(w) @ np.abs(c).T), e=e)
    return scaled(e, w), c, sim.argmax(1).astype(np.int32), scaled(e, sim.max(1))


def topk_reference(x, k):
    """np.sort(...)[:, -k:].mean / .std, the statement of diar_diag.asnorm_scores, in float64."""
    top = np.sort(np.asarray(x, dtype=np.float64), axis=1)[:, -min(k, np.shape(x)[1]):]
    return top.mean(1), top.std(1)


def topk_case(n, k, seed=0, e=0):
    """Rows [7, n] of integers, signs mixed, +0.0 and -0.0 together -> (x, mean, std), NaN where the exact answer is not representable
    (k no power of two and the quotient no integer; a variance that is no perfect square).
      row 0: k / 2 copies of +3 above a long run of -3, the k-th value, of which k / 2 are taken: mean 0, std 3
      row 1: k / 2 copies of 2 above +0.0 and -0.0 mixed, of which k / 2 are taken: mean 1, std 1
      row 2: 1 and -3 in equal numbers (and one -1 when k is odd) above a run of -30: mean -1, std 2 when k is even
      rows 3 ..: random integers in {-9 .. 9}: the k-th value tied many times."""
    register("topk-ties", "gather"), register("topk-int", "dense")
    rng = np.random.default_rng(seed + n + k)
    kk = min(k, n)
    x = rng.integers(-9, 10, (7, n)).astype(np.float64)
    h = kk // 2
    if 2 <= kk < n:
        x[0] = -20.0
        x[0, :h] = 3.0
        x[0, h:h + min(n - h, kk + 30)] = -3.0
        x[1] = -7.0
        x[1, :h] = 2.0
        zeros = min(n - h, kk - h + 9)
        x[1, h:h + zeros] = np.where(np.arange(zeros) % 2, -0.0, 0.0)
    x[2] = -30.0
    x[2, :h] = 1.0
    x[2, h:2 * h] = -3.0
    if kk % 2:
        x[2, 2 * h] = -1.0
    for r in range(3):
        x[r] = x[r, rng.permutation(n)]
    mean, std = topk_reference(x, kk)
    top = np.sort(x, axis=1)[:, -kk:]
    pow2 = (kk & (kk - 1)) == 0
    tot = top.sum(1)
    ss = ((top - mean[:, None]) ** 2).sum(1)
    mean_ok = np.array([pow2 or t % kk == 0 for t in tot])
    need_f32("topk", np.abs(top).sum(1), mean[mean_ok], ((top - mean[:, None]) ** 2)[mean_ok], ss[mean_ok])
    root = np.sqrt(ss / kk)
    std_ok = mean_ok & np.array([(pow2 or s % kk == 0) for s in ss]) & (root * 64 == np.round(root * 64))
    if e:                                                   # the twin: x times 2^e (ldexp keeps the sign of -0.0)
        need_f32("topk", *scaled(e, x, np.abs(top).sum(1), mean[mean_ok]), e=e)
        need_f32("topk", *scaled(2 * e, ((top - mean[:, None]) ** 2)[mean_ok], ss[mean_ok]), e=2 * e)
        x, mean, std = scaled(e, x, mean, std)
    return x, np.where(mean_ok, mean, np.nan), np.where(std_ok, std, np.nan)


def viterbi_scores(T, K, seed=0):
    """Integer scores; every third row (and the first four) constant across the states, so that the dp entries, and with them the
    candidates, tie exactly."""
    register("viterbi-ties", "gather"), register("viterbi-int", "dense")
    rng = np.random.default_rng(seed + T + K)
    s = rng.integers(-3, 4, (T, K)).astype(np.float32)
    s[::3] = rng.integers(-3, 4, (len(range(0, T, 3)), 1))
    s[:4] = 1.0
    return s
