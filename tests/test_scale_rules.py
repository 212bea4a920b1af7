"""The scaled twins of tests/helpers/exact_cases.py and the references of tests/helpers/scale_cases.py, checked without a GPU: the twin
generators against an int64 / float64 restatement and their budget refusals; the numpy statement of the split arithmetic against
float64 -- it keeps the per-value model the pack test asserts, and with all of x at 2^-8 it misses 2^-22 relative, which is the fact
include/sd_hip.h states; the quiet / loud twin of the synthetic network on the CPU oracle."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import exact_cases as E  # noqa: E402
import scale_cases as S  # noqa: E402


def _exponents(name):
    return E.F32_EXPONENTS if E.default_storage(name) == "f32" else E.F16_EXPONENTS


def _restated(c, t, e):
    """The twin's answer from integers: the unscaled operands as int64 multiples of 1 / 2 (the scales are 0.5 .. 4), summed and put
    through the epilogue in int64, then ldexp -- no float64 product or sum of the generator is reused."""
    src = E.source_rows(c.lengths, c.k, c.dil)
    i64 = lambda a: np.round(np.asarray(a) * 2).astype(np.int64)  # noqa: E731
    x, w = np.round(c.x).astype(np.int64), np.round(c.w).astype(np.int64)
    acc = sum(x[src[:, j]] @ w[:, :, j].T for j in range(c.k)) * 2
    if c.bias is not None:
        acc = acc + (np.repeat(i64(c.bias), c.lengths, axis=0) if c.bias_per_seg else i64(c.bias)[None, :])
    if c.act == "relu":
        acc = np.maximum(acc, 0)
    y4 = acc * i64(c.scale)[None, :] + 2 * i64(c.shift)[None, :]          # in quarters
    return np.ldexp(y4.astype(np.float64), e - 2)


@pytest.mark.parametrize("name", E.CONV_CASE_NAMES)
def test_conv_twins_are_ldexp_of_the_case_and_inside_their_budget(name):
    c = E.conv_case(name)
    storages = {"S": ["f32"], "P": ["f32"], "H": ["f16"], "N": ["split"], "W": ["split"]}.get(name[0]) or (
        ["f32"] * (name in E.F32_LABELS) + ["f16"] + ["split"] * (name == "C3x128-256"))
    for storage in storages:
        for e in E.F32_EXPONENTS if storage == "f32" else E.F16_EXPONENTS:
            t = E.conv_case(name, e, storage)
            assert t.e == e and t is E.conv_case(name, e, storage) and np.array_equal(t.w, c.w) and np.array_equal(t.scale if t.scale is not None else 0, c.scale if c.scale is not None else 0)
            assert np.array_equal(t.x, np.ldexp(c.x, e)) and np.array_equal(t.y, np.ldexp(c.y, e))
            assert np.array_equal(t.y, _restated(c, t, e)) if c.scale is not None else True
            if c.tee_hi:
                assert np.array_equal(t.tee, np.ldexp(c.tee, e))
            y32 = t.y.astype(np.float32)
            assert np.array_equal(y32.astype(np.float64), t.y) and (np.abs(y32[y32 != 0]) >= np.finfo(np.float32).tiny).all()
            if storage == "f16":
                for a in (t.x, t.y):
                    assert np.array_equal(a.astype(np.float16).astype(np.float64), a) and np.array_equal(np.round(a * 2.0 ** 24), a * 2.0 ** 24)
            if storage == "split":
                hi, lo = E.split16_halves(t.x)
                assert np.array_equal(hi + lo, t.x)                    # two f16 halves carry x 2^e exactly ...
                if e == -20 and "split_x" in name:                     # ... the low one as a subnormal
                    assert 0 < np.abs(lo[lo != 0]).min() and np.abs(lo).max() < 2.0 ** -14 and (np.abs(hi[hi != 0]) >= 2.0 ** -14).all()
            if name[0] == "C":
                units = E.colstat_units(t)
                base = E.colstat_units(c)
                assert np.array_equal(np.nan_to_num(units[:, :3]), np.ldexp(np.nan_to_num(base[:, :3]), e))
                assert np.array_equal(np.nan_to_num(units[:, 3:]), np.ldexp(np.nan_to_num(base[:, 3:]), 2 * e))
                mean, std = E.colstat_stats(t)
                m0, s0 = E.colstat_stats(c)
                assert np.array_equal(mean, np.ldexp(m0, e)) and np.array_equal(std, np.ldexp(s0, e), equal_nan=True)


def test_f16_twins_reach_the_subnormals_and_the_top_of_the_range():
    """What the three f16 exponents are for: at 2^-20 most stored values are subnormal, at 2^-14 both kinds occur, at 2^4 the largest
    stored value is within a factor 8 of 65504."""
    t = {e: E.conv_case("H2-dense", e) for e in E.F16_EXPONENTS}
    sub = lambda a: (np.abs(a[a != 0]) < 2.0 ** -14).mean()  # noqa: E731
    assert sub(t[-20].x) == 1.0 and sub(t[-20].y) > 0.5 and 0.0 < sub(t[-14].y) < 1.0 and sub(t[4].y) == 0.0
    top = {n: np.abs(E.conv_case(n, 4).y).max() for n in E.CONV_CASE_NAMES if n[0] == "H"}
    assert max(top.values()) * 8 > E.F16_MAX
    with pytest.raises(E.BudgetError, match="exact f16"):              # ... and three binades further the largest case leaves it
        E.conv_case(max(top, key=top.get), 7)
    for bad in (-44, 85):                                           # f32(1e-12) 4^-44 is an f32 subnormal, 4^85 overflows
        with pytest.raises(E.BudgetError, match="normal f32"):
            E.twin_eps(bad)
    for e in E.F32_EXPONENTS + E.F16_EXPONENTS:
        eps = np.float32(E.twin_eps(e))
        assert eps >= np.finfo(np.float32).tiny and float(eps) == float(np.float32(1e-12)) * 4.0 ** e


def test_twin_budgets_refuse_what_leaves_them():
    with pytest.raises(E.BudgetError, match="normal f32"):            # 3 2^-130 is an f32 subnormal
        E.need_f32("t", np.ldexp(np.array([3.0]), -130), e=-130)
    with pytest.raises(E.BudgetError, match="normal f32"):
        E.need_f32("t", np.ldexp(np.array([3.0]), 127), e=127)         # overflows
    with pytest.raises(E.BudgetError, match="exact f32 range"):
        E.need_f32("t", np.ldexp(np.array([2.0 ** 24 + 1]), 12), e=12)  # 25 bits at any scale
    with pytest.raises(E.BudgetError, match="exact f16"):
        E.need_f16("t", np.ldexp(np.array([3.0]), -25), e=-25)         # 3 2^-25 is no multiple of 2^-24
    with pytest.raises(E.BudgetError, match="exact f16"):
        E.need_f16("t", np.ldexp(np.array([2048.0]), 5), e=5)          # 65536
    E.need_f16("t", np.ldexp(np.array([3.0, 1024.0]), -24), e=-24)      # subnormals are exact f16 values
    with pytest.raises(E.BudgetError):
        E.conv_case("S1-dense", 124)                                    # sum |x| |w| 2^124 passes 2^127
    with pytest.raises(E.BudgetError):
        E.conv_case("H1-dense", -26)                                    # half-integers times 2^-26: no multiple of 2^-24
    with pytest.raises(E.BudgetError):
        E.reduction_case(5, 64, 100, e=-70)                             # squares at 4^-70 are f32 subnormals
    with pytest.raises(E.BudgetError):
        E.pool_onehot_case(3, 128, 128, e=-40, f16=True)


@pytest.mark.parametrize("e", E.F32_EXPONENTS + E.F16_EXPONENTS)
def test_reduction_pooling_and_product_twins_are_ldexp_of_the_case(e):
    f16 = e in E.F16_EXPONENTS
    d0, d = E.reduction_case(5, 64, 100, f16=f16), E.reduction_case(5, 64, 100, f16=f16, e=e)
    x = torch.from_numpy(d["x"])
    assert np.array_equal(d["x"], np.ldexp(d0["x"], e)) and np.array_equal(d["gate"], d0["gate"])
    assert np.array_equal(x.mean(1).numpy(), d["mean"]) and np.array_equal(d["y"], d["x"] * d["gate"][:, None] + d["res"])
    ok = ~np.isnan(d["std"]) & (d["std"] != np.ldexp(E.SQRT_EPS, e))
    assert np.array_equal(x.var(1, unbiased=False).sqrt().numpy()[ok], d["std"][ok]) and ok.sum() >= 20
    assert float(np.sqrt(np.float32(d["eps"]))) == np.ldexp(E.SQRT_EPS, e)          # sqrt(eps 4^e) = sqrt(eps) 2^e in f32 as well
    p = E.reduction_case(3, 201, 100, lens=(128,), f16=f16, e=e)
    assert (p["x_poisoned"][:, 128:] == (E.POISON_F16 if f16 else E.POISON)).all() and np.array_equal(p["x"][:, :128].mean(1), p["mean"])
    for fused in (False, True):
        q0 = E.pool_onehot_case(3, 201, 256, lens=(128, 201, 128), fused=fused)
        q = E.pool_onehot_case(3, 201, 256, lens=(128, 201, 128), fused=fused, e=e, f16=f16)
        assert np.array_equal(q["logit"], q0["logit"]) and np.array_equal(q["mean"], np.ldexp(q0["mean"], e))
        assert (q["h"][0, 128:] == E.POISON).all() and (q["h_f16"][0, 128:] == E.POISON_F16).all()
        assert np.array_equal(np.take_along_axis(q["h"], q["tstar"][:, None, :], 1)[:, 0], q["mean"])
    u0, u = E.pool_uniform_case(3, 128, 128), E.pool_uniform_case(3, 128, 128, e=e, f16=f16)
    assert np.array_equal(u["h"].mean(1), u["mean"]) and np.array_equal(u["std"], np.ldexp(u0["std"], e), equal_nan=True)
    if not f16:
        from sklearn.metrics.pairwise import cosine_similarity
        X, K = E.affinity_rows(132, e=e)
        assert np.array_equal(K, E.affinity_rows(132)[1]) and np.array_equal(cosine_similarity(X), K)
        w, c, best, score = E.argmax_case(41, 5, 192, e=e)
        w0, _, best0, score0 = E.argmax_case(41, 5, 192)
        assert np.array_equal(best, best0) and np.array_equal(score, np.ldexp(score0, e)) and np.array_equal((w @ c.T).max(1), score)
        x, mean, std = E.topk_case(257, 64, e=e)
        x0, mean0, std0 = E.topk_case(257, 64)
        assert np.array_equal(np.signbit(x), np.signbit(x0)) and np.array_equal(mean, np.ldexp(mean0, e), equal_nan=True)
        m, s = E.topk_reference(x, 64)
        assert np.array_equal(m[~np.isnan(mean)], mean[~np.isnan(mean)]) and np.array_equal(s[~np.isnan(std)], std[~np.isnan(std)])
    else:
        r0, l0, out0 = E.chain_case("sums", 3, 61, 3)
        r, layers, out = E.chain_case("sums", 3, 61, 3, e=e)
        assert np.array_equal(r, np.ldexp(r0, e)) and np.array_equal(out, np.ldexp(out0, e))
        assert all(np.array_equal(a["bias"], np.ldexp(b["bias"], e)) and np.array_equal(a["w"], b["w"]) for a, b in zip(layers, l0))


# ------------------------------------------------------------------ the split arithmetic in numpy

def test_split_halves_keep_the_per_value_model_of_the_pack_test():
    """|v - (hi + lo)| <= max(2^-22 |v|, 2^-25): relative while lo is a normal f16, absolute once it is subnormal (|v| < 2^-2 or so)."""
    rng = np.random.default_rng(0)
    v = S.f32(rng.standard_normal((64, 400)) * np.logspace(-9, 4, 400)[None, :])
    hi, lo = E.split16_halves(v)
    err = np.abs(hi + lo - np.clip(v, -E.F16_MAX, E.F16_MAX))
    assert (err <= np.maximum(2.0 ** -22 * np.abs(v), 2.0 ** -25)).all()
    big = np.abs(v) >= 0.25
    assert (err[big] <= 2.0 ** -22 * np.abs(v[big])).all()                        # the header's relative promise holds from 2^-2 up
    small = (np.abs(v) < 2.0 ** -8) & (np.abs(v) > 2.0 ** -12)
    assert (err[small] > 2.0 ** -22 * np.abs(v[small])).mean() > 0.5              # ... and not below: most values there miss it
    assert np.array_equal(E.split16_halves(np.array([1e6, -1e6]))[0], [E.F16_MAX, -E.F16_MAX])
    rows = E.split16_rows(v[:, :40])                                               # 40 -> 64 value columns, [hi x 32 | lo x 32]
    assert rows.shape == (64, 128) and np.array_equal(rows[:, 32:40].astype(np.float64), lo[:, :8]) and not rows[:, 72:96].any()


@pytest.mark.parametrize("name", [n for n in E.CONV_CASE_NAMES if "split_" in n])
def test_split_emulation_on_the_twins(name):
    """x side: exact at 2^-20 (hi normal, lo subnormal), and at 2^-26 the answer of 2048 s 2^-26 (lo rounds to zero); w side: the pack's
    2^s absorbs the factor.  The weight scale restated here equals the engine's."""
    from speech_diarization_amd.engine import split16_exponent
    c = E.conv_case(name)
    assert E.split16_weight_shift(c.w) == split16_exponent(c.w.astype(np.float32))
    src = E.source_rows(c.lengths, c.k, c.dil)
    assert np.array_equal(E.split16_conv_sum(c.x, c.w, src), E.conv_sum(c.x, c.w, src))
    if name.endswith("split_x"):
        assert np.array_equal(E.conv_case(name, -20).y, np.ldexp(c.y, -20))
        hi, lo = E.split16_halves(np.ldexp(c.x, -26))
        assert set(np.unique(hi)) == {-2.0 ** -15, 0.0, 2.0 ** -15} and not lo.any()
        t = E.conv_case(name, -26)
        rounded = E.ConvCase(**{**c.__dict__, "x": c.x / 2049.0 * 2048.0, "name": name + "-2048"})
        rounded.bias, rounded.shift, rounded.tee_add = c.bias, c.shift, c.tee_add
        E.conv_epilogue(rounded, E.conv_sum(rounded.x, c.w, src))
        assert np.array_equal(t.y, np.ldexp(rounded.y, -26)) and not np.array_equal(t.y, np.ldexp(c.y, -26))
    else:
        for q in (20, 26):
            t = E.conv_case(name, -q, side="w")
            assert np.array_equal(t.y, np.ldexp(c.y, -q)) and np.array_equal(t.x, c.x)
            assert E.split16_weight_shift(t.w) == E.split16_weight_shift(c.w) + q


def test_split_emulation_misses_the_relative_promise_once_all_of_x_is_small():
    """K = 1024, Gaussian x times 2^e, w ~ N(0, 1 / K): the error of hi.hi + hi.lo + lo.hi against float64, relative to the largest
    output, is f32-level at 2^0 and grows as the low halves turn subnormal -- at 2^-8 it is past 2^-22 and past the 2e-6 of
    test_conv1d_cl_split16_is_as_accurate_as_exact_f32, whose inputs keep 6 channels of 7 at O(1)."""
    rng = np.random.default_rng(3)
    x0 = S.f32(rng.standard_normal((64, 1024)))
    w = S.f32(rng.standard_normal((256, 1024, 1)) / 32.0)
    src = E.source_rows((64,), 1, 1)
    rel = {}
    for e in (0, -4, -8, -12):
        x = np.ldexp(x0, e)
        ref = E.conv_sum(x, w, src)
        rel[e] = np.abs(E.split16_conv_sum(x, w, src) - ref).max() / np.abs(ref).max()
    assert rel[0] < 2.0 ** -22 and rel[-4] < 2e-6
    assert rel[-8] > 2e-6 > 2.0 ** -22 and rel[-12] > 10 * rel[-8] > 100 * rel[0]
    for form in S.ACCURACY_SHAPES:                                     # the shapes of the GPU test: the same trend, and a bar that follows it
        errs = [S.accuracy_bar(*S.accuracy_case(form, e)[4:]) + (np.abs(S.accuracy_case(form, e)[4]).max(),) for e in S.ACCURACY_EXPONENTS]
        assert all(bar == 2 * em + 2e-6 * top for em, bar, top in errs)
        assert errs[0][0] / errs[0][2] < 2e-6 < errs[-1][0] / errs[-1][2]


@pytest.mark.parametrize("side", ["a1", "wc"])
def test_fused_split_case_is_decided_by_the_subnormal_low_half(side):
    """With the halves as the header states them every live logit is exactly 0; with f16 subnormals dropped the odd frames fall by
    2^-16 (2^-18), and the pooled mean of float64 softmax weights moves by far more than an f32 ulp on most channels."""
    B, T, C_, n = 3, 201, 256, 128
    d = E.fused_split_case(B, T, C_, n, side)
    a1, wc = d["a1"].reshape(B * T, -1), d["wc"]
    hi, lo = E.split16_halves(a1) if side == "a1" else E.split16_halves(wc, E.FUSED_WS)
    sub = (lo != 0) & (np.abs(lo) < 2.0 ** -14)
    assert sub.any() and (np.abs(hi[sub]) >= 2.0 ** -14).all()                     # a normal high half over a subnormal low one
    assert not E.fused_split_logits(a1, wc).reshape(B, T, C_)[:, :n].any()
    bad = E.fused_split_logits(a1, wc, flush=True).reshape(B, T, C_)[:, :n]
    assert np.array_equal(bad[:, 0::2], np.zeros_like(bad[:, 0::2])) and (bad[:, 1::2] == -(2.0 ** -16 if side == "a1" else 2.0 ** -18)).all()
    p = np.exp(bad) / np.exp(bad).sum(1, keepdims=True)
    moved = np.abs((p * d["h"][:, :n]).sum(1) - d["mean"])
    assert (moved > 4 * np.spacing(np.abs(d["mean"]).astype(np.float32))).mean() > 0.6
    assert np.array_equal(d["mean"], E.pool_uniform_case(B, T, C_, level=0.0, fused=True, n=n)["mean"]) and (d["h"][:, n:] == E.POISON).all()


# ------------------------------------------------------------------ the quiet / loud twin

def test_scaled_state_dict_is_another_statement_of_the_same_network():
    from oracle import pipeline_ref
    from speech_diarization_amd import synth
    sd = synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(64))
    wav = synth.synthetic_segments(0, 2, 16000)
    base = pipeline_ref.encode_batch_ref(sd, wav, torch.float64)
    for c in (2.0 ** -8, 2.0 ** -4, 2.0, 2.0 ** 5):
        twin = S.scaled_state_dict(sd, c)
        assert set(twin) == set(sd) and all(twin[k].dtype == sd[k].dtype and twin[k].shape == sd[k].shape for k in sd)
        assert np.array_equal(twin["blocks.1.tdnn1.conv.conv.weight"], sd["blocks.1.tdnn1.conv.conv.weight"])
        assert np.array_equal(twin["blocks.1.tdnn1.norm.norm.running_var"], sd["blocks.1.tdnn1.norm.norm.running_var"] * np.float32(c * c))
        assert np.array_equal(twin["asp.tdnn.conv.conv.weight"], sd["asp.tdnn.conv.conv.weight"] / np.float32(c))
        assert np.array_equal(twin["fc.conv.weight"], sd["fc.conv.weight"]) and np.array_equal(twin["asp.tdnn.norm.norm.running_var"], sd["asp.tdnn.norm.norm.running_var"])
        ref = pipeline_ref.encode_batch_ref(twin, wav, torch.float64)
        f32 = pipeline_ref.encode_batch_ref(twin, wav, torch.float32)
        assert np.isfinite(ref).all() and S.cos_dist(f32, ref).max() < 1e-12
        if c >= 2.0:                                                   # BN_EPS is not scaled: the loud twins are the unscaled network to 1e-10
            assert S.cos_dist(ref, base).max() < 1e-9
