"""Parity along the MAGNITUDE axis.  Every other GPU module feeds its kernels values of about 1; here the same kernels, shapes,
selections and launch labels see operands far from 1, f16 subnormals included.

1. Exact twins.  Every case of tests/helpers/exact_cases.py is exact, so its value operands times 2^e must give the bits of
   ldexp(expected, e): the bodies of tests/test_gpu_exact.py run again with `e` (f32 storage: 2^-40, 2^-12, 2^12, 2^40; f16 storage and
   the f16 halves of the split operators: 2^4, 2^-14, 2^-20 -- the top of the range, astride the normal / subnormal edge, mostly
   subnormal), each run under the launch label of its unscaled twin.  No tolerance but that file's own (sqrt(eps) of a constant column).
2. Split twins with subnormal low halves: the 2049 s operand at 2^-20 (hi = 2^-9 normal, lo = 2^-20 an f16 subnormal) and 2^-26 (hi
   subnormal, lo rounds to zero), on the activations (the pack kernel, the narrow kernel's staging split, the SD_DT_SPLIT16 output)
   and on the weights (the host pack absorbs the factor into its 2^s).  The expected values are the header's arithmetic in numpy
   (exact_cases.split16_halves / split16_conv_sum), never a kernel.  The fourth split site, the logits of the fused pooling: a sum
   that cancels to a logit of exactly 0 only if a subnormal low half (of a1, split while staged; of wc 2^8, split in registers)
   takes part, so that the softmax is uniform and the pooled mean exact, or off by tens of ulps (exact_cases.fused_split_case).
3. Rounding does not depend on scale: random f32 inputs, the output at 2^+-12 is ldexp of the same call's output at 2^0 bit for bit (f16
   kernels: f16-exact operands in [2^-2, 2^3) at 2^+-4).  It catches an absolute constant on a rounding path, which integer cases cannot see.
4. The accuracy of the split operators with ALL of x at 2^0 .. 2^-12 against float64, held to twice the error of the numpy emulation
   plus the exact-f32 operator's 2e-6 of the largest output.  Measured (tools/split16_scale.py -> profiles/split16_scale.json).
5. The quiet / loud twin of the synthetic network (scale_cases.scaled_state_dict) through the engine in every precision."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import exact_cases as E  # noqa: E402
import scale_cases as S  # noqa: E402
import test_gpu_exact as X  # noqa: E402
from kernel_selection import CONV_KERNELS, f16_tiles, restore_conv_kernel, select_conv_kernel  # noqa: E402,F401
from launch_log import F16_CONV, F32_CONV, SPLIT_CONV, expect_launches, launches  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16
f32_exp = pytest.mark.parametrize("e", E.F32_EXPONENTS)
f16_exp = pytest.mark.parametrize("e", E.F16_EXPONENTS)
# (storage type, exponent) of the kernels that take both types
BOTH = [(F32, e) for e in E.F32_EXPONENTS] + [(F16, e) for e in E.F16_EXPONENTS]
both_exp = pytest.mark.parametrize("dtype,e", BOTH)
MODES = [("f32", e) for e in E.F32_EXPONENTS] + [("split16", e) for e in E.F32_EXPONENTS] + [("f16", e) for e in E.F16_EXPONENTS]
mode_exp = pytest.mark.parametrize("mode,e", MODES)


# ------------------------------------------------------------------ 1. exact twins at 2^e

@f32_exp
@pytest.mark.parametrize("name", X.F32_CASES)
def test_conv1d_cl_f32_twin(dev, name, e):
    X.test_conv1d_cl_f32_every_selection_gives_the_integers(dev, name, e=e)


@f32_exp
@pytest.mark.parametrize("name", ["P-rows", "P-chan", "P-dense"])
def test_conv1d_cl_packed_f32_twin(dev, name, e):
    X.test_conv1d_cl_packed_f32_gives_the_integers(dev, name, e=e)


@f16_exp
@pytest.mark.parametrize("name", X.F16_CASES)
def test_conv1d_cl_f16_twin(dev, f16_tiles, name, e):
    """x, y, tee and tee_add as f16 at 2^e: at 2^-20 every one of them an f16 subnormal."""
    X.test_conv1d_cl_f16_gives_the_integers(dev, f16_tiles, name, e=e)


@f16_exp
@pytest.mark.parametrize("name", [n for n in E.CONV_CASE_NAMES if n[0] in "NW"])
def test_conv1d_cl_split16_twin(dev, name, e):
    """The activations are carried as f16 halves, so they take the f16 exponents; y is f32, or SD_DT_SPLIT16 compared with the numpy pack."""
    X.test_conv1d_cl_split16_gives_the_integers(dev, name, e=e)


@f32_exp
@pytest.mark.parametrize("name", ["C3x128-256", "C5x64-256"])
def test_colstat_f32_twin(dev, name, e):
    """The pivot is the scaled shift, the sums of squares scale by 4^e, eps = 1e-12 4^e."""
    X.test_colstat_f32_gives_the_integer_sums(dev, name, e=e)


@f16_exp
@pytest.mark.parametrize("name", ["C3x128-256", "C5x64-256", "C11x64-1024", "C3x128-1024"])
def test_colstat_f16_twin(dev, f16_tiles, name, e):
    X.test_colstat_f16_gives_the_integer_sums(dev, f16_tiles, name, e=e)


@f16_exp
def test_colstat_split16_twin(dev, e):
    X.test_colstat_split16_gives_the_integer_sums(dev, e=e)


@f16_exp
@pytest.mark.parametrize("kind", ["onehot", "sums"])
@pytest.mark.parametrize("B,T,dil", E.CHAIN_SHAPES)
def test_res2net_chain_f16_twin(dev, kind, B, T, dil, e):
    """Every chain state y_j and c_{j+1} + y_j at 2^e, fused and as seven unfused convs."""
    X.test_res2net_chain_f16_gives_the_integer_chain(dev, kind, B, T, dil, e=e)


@both_exp
@pytest.mark.parametrize("B,T,C_", X.REDUCE_SHAPES)
def test_seg_mean_std_and_se_scale_residual_twin(dev, dtype, e, B, T, C_):
    X.test_seg_mean_std_and_se_scale_residual_uniform(dev, dtype, B, T, C_, e=e)


@both_exp
@pytest.mark.parametrize("T,n", E.LENS)
def test_seg_mean_std_with_lens_twin(dev, dtype, e, T, n):
    X.test_seg_mean_std_with_lens_ignores_the_padded_frames(dev, dtype, T, n, e=e)


@both_exp
def test_seg_mean_std_and_se_scale_residual_packed_twin(dev, dtype, e):
    X.test_seg_mean_std_and_se_scale_residual_packed(dev, dtype, e=e)


@both_exp
@pytest.mark.parametrize("B,T,C_", X.POOL_SHAPES)
def test_asp_pool_one_hot_twin(dev, dtype, e, B, T, C_):
    """h at 2^e, the logits as they are."""
    X.test_asp_pool_one_hot_logits_return_one_frame(dev, dtype, B, T, C_, e=e)


@both_exp
@pytest.mark.parametrize("B,T,C_", [(3, 128, 128), (3, 256, 128), (3, 64, 100)])
def test_asp_pool_uniform_twin(dev, dtype, e, B, T, C_):
    X.test_asp_pool_uniform_weights_give_the_exact_mean_and_std(dev, dtype, B, T, C_, e=e)


@both_exp
@pytest.mark.parametrize("T,n", E.LENS)
@pytest.mark.parametrize("C_", [128, 100])
def test_asp_pool_with_lens_twin(dev, dtype, e, T, n, C_):
    X.test_asp_pool_with_lens_ignores_the_padded_frames(dev, dtype, T, n, C_, e=e)
    X.test_asp_pool_with_lens_uniform_weights_over_the_live_frames(dev, dtype, T, n, C_, e=e)


@both_exp
def test_asp_pool_packed_twin(dev, dtype, e):
    X.test_asp_pool_packed_one_hot(dev, e=e, dtypes=(dtype,))


@mode_exp
@pytest.mark.parametrize("T", X.FUSED_T)
def test_fused_attention_pooling_one_hot_twin(dev, mode, e, T):
    X.test_fused_attention_pooling_one_hot(dev, mode, T, e=e)


@mode_exp
@pytest.mark.parametrize("T", [64, 128, 256])
def test_fused_attention_pooling_uniform_twin(dev, mode, e, T):
    X.test_fused_attention_pooling_uniform_weights(dev, mode, T, e=e)


@mode_exp
@pytest.mark.parametrize("T,n", E.LENS)
def test_fused_attention_pooling_with_lens_twin(dev, mode, e, T, n):
    X.test_fused_attention_pooling_with_lens_ignores_the_padded_frames(dev, mode, T, n, e=e)
    X.test_fused_attention_pooling_with_lens_uniform_weights_over_the_live_frames(dev, mode, T, n, e=e)


@f32_exp
@pytest.mark.parametrize("n", [132, 1412])
def test_cosine_affinity_of_scaled_rows_keeps_its_bits(dev, n, e):
    """Every row times 2^e: l2norm gives the unit rows of the unscaled case, so both kernels (exact f32 and split16x3, which scales its
    unit rows by 16 whatever the input's size) must return the bits of k / 16."""
    X.test_cosine_affinity_is_k_over_16(dev, n, e=e)


@f32_exp
@pytest.mark.parametrize("K", [1, 5, 64])
@pytest.mark.parametrize("N_", [1, 41, 130])
@pytest.mark.parametrize("D", [7, 192, 200])
def test_sim_argmax_twin(dev, K, N_, D, e):
    """The same index, the score times 2^e."""
    X.test_sim_argmax_returns_the_first_maximum(dev, K, N_, D, e=e)


@f32_exp
def test_adjacent_cosine_and_l2norm_rows_twin(dev, e):
    X.test_adjacent_cosine_and_l2norm_rows_are_exact(dev, e=e)


@f32_exp
@pytest.mark.parametrize("n", [50, 257, 1000])
@pytest.mark.parametrize("k", [1, 64, "n"])
def test_topk_mean_std_twin(dev, n, k, e):
    X.test_topk_mean_std_on_tied_integer_rows(dev, n, k, e=e)


# ------------------------------------------------------------------ 2. split twins with subnormal lows

SPLIT_Q = (20, 26)


@pytest.mark.parametrize("q", SPLIT_Q)
@pytest.mark.parametrize("name", [n for n in E.CONV_CASE_NAMES if n.endswith("split_x")])
def test_split_x_with_subnormal_lows(dev, name, q):
    """x = 2049 s 2^-q.  q = 20: (2^-9, 2^-20), the low half an f16 subnormal; q = 26: hi = 2^-15 is subnormal and lo rounds to zero,
    so the operator computes with 2048 s 2^-26 -- the expected y is what the halves give, not ldexp of the unscaled answer.  W*: the
    pack kernel; N128: the staging split of the narrow kernel; where cout % 32 == 0 also y as SD_DT_SPLIT16 against the numpy pack."""
    X.test_conv1d_cl_split16_gives_the_integers(dev, name, e=-q)


@pytest.mark.parametrize("q", SPLIT_Q)
@pytest.mark.parametrize("name", [n for n in E.CONV_CASE_NAMES if n.endswith("split_w")])
def test_split_w_scaled_is_absorbed_by_the_host_pack(dev, name, q):
    """w = 2049 s 2^-q (bias, shift and tee_add with it, x as it is): the pack's 2^s takes the factor, y is ldexp of the unscaled one."""
    want = E.conv_case(name)
    assert np.array_equal(E.conv_case(name, -q, side="w").y, np.ldexp(want.y, -q))
    X.test_conv1d_cl_split16_gives_the_integers(dev, name, e=-q, side="w")


@pytest.mark.parametrize("e", (4, -14, -20, -26))
def test_split16_pack_equals_the_numpy_pack(dev, e):
    """sd_split16_pack_f32 on 2049 s 2^e and on small integers 2^e (a slice of a wider row, 80 -> 96 value columns), as bits."""
    from speech_diarization_amd import ops
    for name in ("W1032-split_x", "W1032-rows"):
        x = E.scaled(e, E.conv_case(name).x)
        xbuf, _ = X._framed(x, F32, dev)
        with expect_launches(exactly=["split16_pack_kernel"]):
            got = ops.split16_pack(xbuf, 8, x.shape[1])
            torch.cuda.synchronize()
        X._same(got, torch.from_numpy(E.split16_rows(x)), f"split16_pack {name} 2^{e}")
    hi, lo = E.split16_halves(E.scaled(e, np.array([2049.0])))
    assert (hi[0], lo[0]) == {4: (32768.0, 16.0), -14: (2.0 ** -3, 2.0 ** -14), -20: (2.0 ** -9, 2.0 ** -20), -26: (2.0 ** -15, 0.0)}[e]


@pytest.mark.parametrize("side", ["a1", "wc"])
@pytest.mark.parametrize("T,n", [(64, 64), (128, 128), (201, 128), (256, 256)])
def test_fused_split_logits_keep_a_subnormal_low_half(dev, side, T, n):
    """Every template of the split kernel (16-frame tiles x 4, 8, 13, 16; T = 201 with 128 live frames through the relative lengths).
    The odd frames' logit is 0 only with the subnormal half in the product; then the answer is the exact mean and std of the
    uniform case.  A kernel that flushed it, in the staging split, in the register split or in the MFMA, would weigh the odd frames
    2^-16 (2^-18) lower and miss the mean of the 0 / 2 columns by tens of ulps."""
    B, C_ = 3, 256
    d = E.fused_split_case(B, T, C_, n, side)
    rel = None if n == T else torch.full((B,), float(E.rel_len(T, n)), device=dev)
    got = X._attend(dev, "split16", d["a1"], d["wc"], d["h"], B, T, C_, rel)
    X._check_stats(got, d["mean"], d["std"], C_, f"fused split logits {side} T={T} n={n}", dev)


# ------------------------------------------------------------------ 3. rounding does not depend on scale

ID_EXP = (12, -12)


def _identity(dev, run, c, exps, what):
    """run(case) -> dict of outputs; every output at 2^e must be the output at 2^0 times 2^e, bit for bit."""
    base = run(c)
    for e in exps:
        got = run(S.at_scale(c, e))
        for k, v in got.items():
            X._same(v, base[k] * 2.0 ** e, f"{what} {k} at 2^{e} against ldexp of 2^0")


@pytest.mark.parametrize("name", [n for n in E.DENSE if n[0] == "S"])
def test_f32_conv_rounding_does_not_depend_on_scale(dev, name):
    """sd_conv1d_cl_f32 under every selection (and S4 through sd_seg_gemm_f32), held to the labels of the exact cases."""
    c = S.random_conv(name)
    try:
        for sel in CONV_KERNELS:
            select_conv_kernel(sel)

            def run(t):
                with expect_launches(exactly=[E.F32_LABELS[name.split("-")[0]][sel]], family=F32_CONV):
                    return X.run_conv(dev, t, "f32")
            _identity(dev, run, c, ID_EXP, f"{name} {sel}")
    finally:
        restore_conv_kernel()
    if name.startswith("S4"):
        def seg(t):
            with expect_launches(exactly=E.SEG_GEMM_LABELS, family=F32_CONV):
                return X.run_conv(dev, t, "seg")
        _identity(dev, seg, c, ID_EXP, f"{name} seg_gemm")


def test_packed_f32_conv_rounding_does_not_depend_on_scale(dev):
    def run(t):
        with expect_launches(exactly=[E.PACKED_LABEL], family=F32_CONV):
            return X.run_conv(dev, t, "packed")
    _identity(dev, run, S.random_conv("P-dense"), ID_EXP, "P-dense packed")


@pytest.mark.parametrize("name", [n for n in E.DENSE if n[0] == "H"])
def test_f16_conv_rounding_does_not_depend_on_scale(dev, f16_tiles, name):
    """f16-exact operands in [2^-2, 2^3) at 2^+-4, y as f16 and as f32: see scale_cases.random_conv for why no stored value is subnormal."""
    c = S.random_conv(name, f16=True)
    for xdt in (F16, F32):
        for ydt in (F16, F32):
            def run(t):
                with expect_launches(exactly=[E.f16_label(name, f16_tiles, xdt == F16, ydt == F16)], family=F16_CONV):
                    return X.run_conv(dev, t, "f16", xdt, ydt)
            _identity(dev, run, c, (4, -4), f"{name} {f16_tiles} x {xdt} y {ydt}")


@pytest.mark.parametrize("B,T,dil", [(3, 61, 3), (2, 212, 4)])
def test_res2net_chain_rounding_does_not_depend_on_scale(dev, B, T, dil):
    from speech_diarization_amd import ops
    r, layers = S.random_chain(B, T, dil)

    def run(e):
        dl = [dict(w=ops.pack_weight(L["w"], dev, F16), bias=X._dev(E.scaled(e, L["bias"]), F32, dev), scale=X._dev(L["scale"], F32, dev),
                   shift=X._dev(E.scaled(e, L["shift"]), F32, dev), dil=dil) for L in layers]
        got = X._dev(E.scaled(e, r), F16, dev)
        with expect_launches(exactly=["chain_pack_kernel", f"res2net_chain_f16_kernel<{(T + 31) // 32}>"]):
            ops.res2net_chain(got, T, dl)
            torch.cuda.synchronize()
        return got
    base = run(0)
    assert float(base[:, 128:1024].min()) >= 1.0 and float(base.max()) < 2.0 ** 11       # no subnormal at 2^-4, no overflow at 2^4
    for e in (4, -4):
        X._same(run(e), base * 2.0 ** e, f"chain T={T} at 2^{e}")


def _random_stats_inputs(B, T, C_, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B * T, C_, generator=g), torch.randn(B * T, C_, generator=g)


@pytest.mark.parametrize("B,T,C_", X.REDUCE_SHAPES)
def test_seg_mean_std_rounding_does_not_depend_on_scale(dev, B, T, C_):
    from speech_diarization_amd import ops
    x, _ = _random_stats_inputs(B, T, C_, T + C_)
    with expect_launches(exactly=[f"seg_mean_std_kernel<f32,uniform,{X.REDUCE_FORM[B, T, C_]}>"]):
        base = ops.seg_mean_std(x.to(dev), B, T)
        for e in ID_EXP:
            got = ops.seg_mean_std((x * 2.0 ** e).to(dev), B, T, eps=E.twin_eps(e))
            X._same(got, base * 2.0 ** e, f"seg_mean_std at 2^{e}")


@pytest.mark.parametrize("B,T,C_", X.POOL_SHAPES)
def test_asp_pool_rounding_does_not_depend_on_scale(dev, B, T, C_):
    """Both kernels (LDS-resident and streaming): random logits of about 1, h at 2^e, eps 4^e."""
    from speech_diarization_amd import ops
    logit, h = _random_stats_inputs(B, T, C_, T + C_)
    with expect_launches(exactly=[X._pool_label(F32, T, C_)], family=X.POOL_FAMILY):
        base = ops.asp_pool(logit.to(dev), h.to(dev), B, T)
        for e in ID_EXP:
            got = ops.asp_pool(logit.to(dev), (h * 2.0 ** e).to(dev), B, T, eps=E.twin_eps(e))
            X._same(got, base * 2.0 ** e, f"asp_pool T={T} C={C_} at 2^{e}")


@pytest.mark.parametrize("T", [64, 129, 208, 256])
def test_fused_f32_pooling_rounding_does_not_depend_on_scale(dev, T):
    from speech_diarization_amd import ops
    B, C_, att = 3, 256, 128
    g = torch.Generator().manual_seed(T)
    a1, h = torch.randn(B * T, att, generator=g), torch.randn(B * T, C_, generator=g)
    wc = ops.pack_weight(torch.randn(C_, att, 1, generator=g) / np.sqrt(att), dev)
    with expect_launches(exactly=[X._fused_label("f32", T)], family={"asp_attend_pool_f32_kernel", "asp_attend_pool_f16_kernel"}):
        base = ops.asp_attend_pool(a1.to(dev), wc, h.to(dev), B, T)
        for e in ID_EXP:
            got = ops.asp_attend_pool(a1.to(dev), wc, (h * 2.0 ** e).to(dev), B, T, eps=E.twin_eps(e))
            X._same(got, base * 2.0 ** e, f"fused f32 pooling T={T} at 2^{e}")


def test_colstat_and_finish_rounding_does_not_depend_on_scale(dev):
    """(3, 128) x 256 under every selection: the raw units scale by 2^e (sums) and 4^e (sums of squares), mean and std by 2^e."""
    from speech_diarization_amd import ops
    B, T, cin, cout = 3, 128, 64, 256
    rng = np.random.default_rng(5)
    c = E.ConvCase("C3x128-256-random", "dense", (T,) * B, False, cin, cout, 1, 1, S.f32(rng.standard_normal((B * T, cin))),
                   S.f32(rng.standard_normal((cout, cin, 1)) / 8.0), bias=S.f32(rng.standard_normal(cout)), act="relu",
                   scale=S.f32(rng.uniform(0.5, 1.5, cout)), shift=S.f32(rng.standard_normal(cout)))
    n_cs = ops.colstat_floats(c.M, cout)
    try:
        for sel in CONV_KERNELS:
            select_conv_kernel(sel)

            def run(t, e):
                cs = torch.full((n_cs,), float("nan"), device=dev)
                with expect_launches(exactly=[E.F32_LABELS["C3x128-256"][sel]], family=F32_CONV):
                    y = X.run_conv(dev, t, "f32", colstat=cs)["y"].contiguous()
                with expect_launches(exactly=["colstat_finish_kernel<f32>"]):
                    st = ops.colstat_finish(cs, y, B, T, pivot=X._dev(t.shift, F32, dev), want_std=True, eps=E.twin_eps(e))
                return y, cs.view(-1, 6, cout), st
            y0, cs0, st0 = run(c, 0)
            for e in ID_EXP:
                y, cs, st = run(S.at_scale(c, e), e)
                X._same(y, y0 * 2.0 ** e, f"{sel} y at 2^{e}")
                X._same(torch.nan_to_num(cs[:, :3]), torch.nan_to_num(cs0[:, :3]) * 2.0 ** e, f"{sel} colstat sums at 2^{e}")
                X._same(torch.nan_to_num(cs[:, 3:]), torch.nan_to_num(cs0[:, 3:]) * 4.0 ** e, f"{sel} colstat sums of squares at 2^{e}")
                X._same(st, st0 * 2.0 ** e, f"{sel} colstat_finish at 2^{e}")
    finally:
        restore_conv_kernel()


# ------------------------------------------------------------------ 4. accuracy of the split operators as a function of scale

@pytest.mark.parametrize("e", S.ACCURACY_EXPONENTS)
@pytest.mark.parametrize("form", ["wide", "narrow"])
def test_split16_accuracy_follows_the_emulated_model_at_every_scale(dev, form, e):
    """Every channel of x at 2^e.  Below 2^-2 the low halves are f16 subnormals and the representation error is 2^-25 absolute per
    value (include/sd_hip.h), so the error relative to the largest output grows as the scale falls; the kernel must stay within twice
    the error of the header's arithmetic in numpy, plus 2e-6 of the largest output.  An f16 MFMA or a pack that flushed subnormals
    would lose the low halves altogether."""
    labels = E.split_labels("W1024-chan") if form == "wide" else E.split_labels("N128-chan")      # cout 1024, plain epilogue: the register form
    with expect_launches(exactly=labels, family=SPLIT_CONV):
        r = S.measure_accuracy(dev, form, e)
    print(f"\n[{form} x 2^{e}] error vs float64: kernel {r['measured']:.3e}, emulation {r['emulated']:.3e}, bar {r['bar']:.3e}; "
          f"relative to the largest output {r['top']:.3e}: {r['measured'] / r['top']:.2e} / {r['emulated'] / r['top']:.2e}")
    assert r["measured"] <= r["bar"], r


# ------------------------------------------------------------------ 5. the quiet / loud twin of the network

@pytest.fixture(scope="module")
def twin_inputs():
    from oracle import pipeline_ref
    from speech_diarization_amd import synth
    sd = synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(128))
    wav = synth.synthetic_segments(0, 3, 16000)
    twins = {c: S.scaled_state_dict(sd, c) for c in S.ENGINE_SCALES}
    return wav, twins, {c: pipeline_ref.encode_batch_ref(t, wav, torch.float64) for c, t in twins.items()}


@pytest.mark.parametrize("precision", S.ENGINE_PRECISIONS)
@pytest.mark.parametrize("c", S.ENGINE_SCALES)
def test_engine_on_the_quiet_and_the_loud_twin(dev, twin_inputs, c, precision):
    """All frame-level activations at c = 2^-8 and 2^5 times their size, against the float64 oracle on the same twin; the suite's own
    bars (cosine distance 1e-5; f16: 1e-3).  What this geometry reaches, as the launch log states it: three segments of width 128 are
    small launches, which the schedule keeps on the exact-f32 kernels under "f32ns" (the same launches as "f32", hence the same
    bits) and sends to the narrow split kernel alone under "f32s"; the pack kernel, the 256x256 split form and the fused split
    pooling do not see this twin -- their behaviour at 2^e is pinned per operator above."""
    from speech_diarization_amd.engine import EmbeddingEngine
    wav, twins, refs = twin_inputs
    eng = EmbeddingEngine(twins[c], dev, precision=precision)
    with launches() as log:
        got = eng.embed(torch.from_numpy(wav).to(dev)).cpu().numpy()
    cd = S.cos_dist(got, refs[c])
    split = sorted(lb for lb in log if "split" in lb)
    print(f"\n[{precision} c = {c:g}] cosine distance to float64: {cd.max():.3e}; split launches: {split}")
    assert (split == ["conv_gemm_split16_n128_kernel"]) if precision == "f32s" else not split, (precision, split)
    assert np.isfinite(got).all() and cd.max() < (1e-3 if precision == "f16" else 1e-5), cd
