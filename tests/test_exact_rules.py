"""The known-answer cases of tests/helpers/exact_cases.py, checked without a GPU: every integer reference against independent arithmetic
(torch conv1d with reflect padding in float64, sklearn, the numpy stand-ins of ahc_ref / spectral_ref, the numpy statements of
diar_diag.py) -- EXACTLY equal, not close; every case inside its bit budget and an oversized one refused; `EXACT_COVERAGE` complete over kernels and over launch labels; and
the expected values reachable in the kernels' own arithmetic (torch f32, the split16 hi / lo decomposition and the three-product sum)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ahc_ref  # noqa: E402
import exact_cases as E  # noqa: E402
import kernel_census  # noqa: E402
import kernel_selection  # noqa: E402
import spectral_ref  # noqa: E402


def _conv1d_ref(c, dtype=torch.float64):
    """F.conv1d over each segment with F.pad(mode="reflect"), then the epilogue, in `dtype`."""
    x, w = torch.from_numpy(c.x).to(dtype), torch.from_numpy(c.w).to(dtype)
    pad = c.dil * (c.k - 1) // 2
    out, start = [], 0
    for L in c.lengths:
        xt = x[start:start + L].T[None]
        if pad:
            xt = F.pad(xt, (pad, pad), mode="reflect")
        out.append(F.conv1d(xt, w, dilation=c.dil)[0].T)
        start += L
    y = torch.cat(out)
    if c.bias is not None:
        b = torch.from_numpy(c.bias).to(dtype)
        y = y + (torch.repeat_interleave(b, torch.tensor(c.lengths), dim=0) if c.bias_per_seg else b)
    if c.act == "relu":
        y = torch.relu(y)
    y = y * torch.from_numpy(c.scale).to(dtype) + torch.from_numpy(c.shift).to(dtype) if c.scale is not None else y
    tee = None
    if c.tee_hi:
        tee = y[:, c.tee_lo:c.tee_hi] + (torch.from_numpy(c.tee_add).to(dtype) if c.tee_add is not None else 0)
    return y, tee


# ------------------------------------------------------------------ 1. references against independent arithmetic

@pytest.mark.parametrize("name", E.CONV_CASE_NAMES)
def test_conv_reference_equals_torch_conv1d_in_float64(name):
    c = E.conv_case(name)
    y, tee = _conv1d_ref(c)
    assert np.array_equal(y.numpy(), c.y)
    if c.tee_hi:
        assert np.array_equal(tee.numpy(), c.tee)
    assert c.M == sum(c.lengths) and c.y.shape == (c.M, c.cout) and tuple(c.kernels) == E.CASE_TABLE[name][1]


@pytest.mark.parametrize("name", [n for n in E.CONV_CASE_NAMES if n.endswith("-rows")])
def test_row_gather_names_the_reflected_source_row(name):
    """Every tap is used, both segment ends reflect, and no source row leaves its own segment."""
    c = E.conv_case(name)
    seg = np.repeat(np.arange(c.B), c.lengths)
    src = c.y.astype(np.int64)
    assert np.array_equal(seg[src], np.repeat(seg[:, None], c.cout, 1))
    assert set(np.unique(np.argmax(c.w.reshape(c.cout, c.cin, c.k).sum(1), axis=1))) == set(range(c.k))
    if c.k > 1:
        m = np.arange(c.M)[:, None]
        assert (src > m).any() and (src < m).any() and (src[0] > 0).any() and (src[c.M - 1] < c.M - 1).any()
    used = np.unique(np.argmax(c.w.sum(2), axis=1))
    assert 0 in used and c.cin - 1 in used


def test_colstat_cases_have_the_statistics_they_were_built_for():
    for name in ("C3x128-256", "C5x64-256", "C11x64-1024", "C3x128-1024"):
        c = E.conv_case(name)
        v = (c.y - c.shift).reshape(c.B, c.T, c.cout)
        assert v.min() == 0 and v.max() == 3
        mean, std = E.colstat_stats(c)
        n = np.arange(c.cout)
        assert np.array_equal(std[:, n % 3 == 0], np.ones((c.B, (n % 3 == 0).sum())))
        assert np.all(std[:, n % 3 == 1] == E.SQRT_EPS) and abs(E.SQRT_EPS - 1e-6) <= 1e-6 * 1e-6
        units = E.colstat_units(c)
        assert np.array_equal(np.nansum(units[:, :3], axis=(0, 1)), v.sum((0, 1)))
        assert np.array_equal(np.nansum(units[:, 3:], axis=(0, 1)), (v * v).sum((0, 1)))
        assert np.array_equal(mean, c.shift[None, :] + v.mean(1))


@pytest.mark.parametrize("kind", ["onehot", "sums"])
@pytest.mark.parametrize("B,T,dil", E.CHAIN_SHAPES)
def test_chain_reference_equals_seven_torch_convs(kind, B, T, dil):
    r, layers, want = E.chain_case(kind, B, T, dil)
    rt = torch.from_numpy(r).clone()
    u = rt[:, 128:256].clone()
    for j, L in enumerate(layers, 1):
        xt = F.pad(u.view(B, T, 128).transpose(1, 2), (dil, dil), mode="reflect")
        y = F.conv1d(xt, torch.from_numpy(L["w"]), torch.from_numpy(L["bias"]), dilation=dil).transpose(1, 2).reshape(B * T, 128)
        y = torch.relu(y) * torch.from_numpy(L["scale"]) + torch.from_numpy(L["shift"])
        assert torch.equal(y.half().double(), y)                       # every chain state an exact f16
        rt[:, 128 * j:128 * j + 128] = y
        if j < len(layers):
            u = y + torch.from_numpy(r[:, 128 * (j + 1):128 * (j + 2)])
            assert torch.equal(u.half().double(), u)
    assert np.array_equal(rt.numpy(), want)
    assert np.array_equal(want[:, :128], r[:, :128]) and np.array_equal(want[:, 1024:], r[:, 1024:])


@pytest.mark.parametrize("n", [4, 132, 260, 1030, 1412])
def test_affinity_reference_equals_sklearn(n):
    from sklearn.metrics.pairwise import cosine_similarity
    X, K = E.affinity_rows(n)
    assert np.array_equal(cosine_similarity(X), K) and np.array_equal(cosine_similarity(X.astype(np.float32)), K.astype(np.float32))
    assert np.array_equal(K * 16, np.round(K * 16)) and not K[2].any() and K[0, 1] == 1 and K[0, n - 1] == 1
    assert set(np.abs(X).sum(1)) == {0.0, 16.0}


@pytest.mark.parametrize("n,d", [(129, 7), (257, 190), (300, 192)])
def test_ahc_reference_equals_the_numpy_stand_in(n, d):
    S, count, inv, nn, best = E.ahc_case(n, d, d + 8)
    nn_ref, best_ref = ahc_ref.nearest_f32(S[:, :d], inv)
    assert np.array_equal(nn_ref, nn) and np.array_equal(best_ref, best.astype(np.float32))
    score = ahc_ref.scores_f64(S[:, :d], inv)
    ties = (score == score.max(1, keepdims=True)).sum(1)
    assert (ties > 1).mean() > 0.5                                   # nearly every row has several equal best scores
    assert np.isnan(S[:, d:]).all()


@pytest.mark.parametrize("n,b", [(129, 8), (600, 24), (1030, 32)])
@pytest.mark.parametrize("onehot", [False, True])
def test_spectral_reference_equals_the_f64_reference(n, b, onehot):
    K, scale, V = E.spectral_case(n, b, n + 5, onehot=onehot)
    for zero_diag in (False, True):
        deg, Y = E.spectral_expected(K, scale, V, zero_diag)
        assert np.array_equal(deg, spectral_ref.degree_ref(K[:, :n], zero_diag))
        assert np.array_equal(Y, spectral_ref.apply_ref(K[:, :n], scale, V, zero_diag)[0])
        assert np.array_equal(Y.astype(np.float32).astype(np.float64), Y)
    if onehot:
        js = V.argmax(0)
        assert js[0] == 0 and js[-1] == n - 1
        assert np.array_equal(E.spectral_expected(K, scale, V, False)[1], scale[:, None] * np.clip(K[:, js], 0, None) * scale[js][None, :])


@pytest.mark.parametrize("n", [50, 257, 1000])
@pytest.mark.parametrize("k", [1, 64, 0])
def test_topk_reference_is_the_numpy_statement(n, k):
    """diar_diag.asnorm_scores: np.sort(scores, axis=1)[:, -k:] then .mean / .std."""
    k = k or n
    x, mean, std = E.topk_case(n, k)
    qc = np.sort(x.astype(np.float32), axis=1)[:, -min(k, n):].astype(np.float64)
    ok_m, ok_s = ~np.isnan(mean), ~np.isnan(std)
    assert np.array_equal(qc.mean(axis=1)[ok_m], mean[ok_m]) and np.array_equal(qc.std(axis=1)[ok_s], std[ok_s])
    assert ok_m.any() and (ok_m.all() if (min(k, n) & (min(k, n) - 1)) == 0 else True)
    if 2 <= k < n:
        kth = qc[:, 0]
        assert ((x == kth[:, None]).sum(1) > 1).all()                  # the k-th value is tied in every row
        assert (mean[0], std[0], mean[1], std[1]) == (0.0, 3.0, 1.0, 1.0)
        assert np.signbit(x[1][x[1] == 0]).any() and not np.signbit(x[1][x[1] == 0]).all()     # +0.0 and -0.0 together
    assert mean[2] == -1.0 and (std[2] == 2.0 or min(k, n) % 2)
    assert (x < 0).any(1).all() and (k == 1 or (x > 0).any(1).all())              # signs mixed: the ordered-key map flips at 0


def _viterbi_restated(scores, alpha):
    """The recurrence of diar_diag.viterbi_hmm in plain loops over f32 values: first maximum wins."""
    T, K = scores.shape
    move = np.float32(np.log((1 - alpha) / (K - 1) + 1e-8)) if K > 1 else np.float32(0.0)
    stay = np.float32(np.log(alpha + 1e-8))
    dp = scores[0].astype(np.float32).copy()
    back = np.zeros((T, K), dtype=np.int32)
    ties = 0
    for t in range(1, T):
        new = np.empty(K, dtype=np.float32)
        for j in range(K):
            best, arg = np.float32(-np.inf), 0
            for i in range(K):
                cand = np.float32(dp[i] + (stay if i == j else move))
                ties += int(cand == best)
                if cand > best:
                    best, arg = cand, i
            back[t, j] = arg
            new[j] = np.float32(best + scores[t, j])
        dp = new
    path = np.zeros(T, dtype=np.int32)
    path[-1] = int(np.argmax(dp))
    for t in range(T - 2, -1, -1):
        path[t] = back[t + 1, path[t + 1]]
    return path, ties


@pytest.mark.parametrize("T,K", [(1, 2), (2, 8), (129, 8), (130, 2), (40, 64)])
def test_viterbi_reference_and_its_ties(T, K):
    from speech_diarization_amd import diar_diag
    s = E.viterbi_scores(T, K)
    assert np.array_equal(s, np.round(s)) and (s[::3] == s[::3, :1]).all()
    for alpha in (0.9, 0.995, 0.01):
        path, ties = _viterbi_restated(s, alpha)
        assert np.array_equal(diar_diag.viterbi_hmm(s, alpha), path)
        assert T < 3 or ties > 0
    if K == 8:
        assert 0.01 < 1.0 / K                                         # moving beats staying: every i != j candidate ties on a flat dp


def test_reduction_and_pooling_references():
    for T, n in E.LENS:
        from speech_diarization_amd.features import length_frames
        n_norm, n_mask = length_frames(torch.tensor([float(E.rel_len(T, n))]), T)
        assert int(n_norm) == n and int(n_mask) == n
    d = E.reduction_case(5, 64, 100)
    x = torch.from_numpy(d["x"])
    assert np.array_equal(x.mean(1).numpy(), d["mean"])
    sd = x.var(1, unbiased=False).sqrt().numpy()
    ok = ~np.isnan(d["std"]) & (d["std"] != E.SQRT_EPS)
    assert np.array_equal(sd[ok], d["std"][ok]) and ok.sum() >= 20 and (d["std"] == E.SQRT_EPS).sum() >= 20
    assert np.array_equal((x * torch.from_numpy(d["gate"])[:, None] + torch.from_numpy(d["res"])).numpy(), d["y"])
    d = E.reduction_case(3, 201, 100, lens=(128,))
    assert np.array_equal(d["x"][:, :128].mean(1), d["mean"]) and (d["x_poisoned"][:, 128:] == E.POISON).all()
    for fused in (False, True):
        p = E.pool_onehot_case(3, 201, 256, lens=(128, 201, 128), fused=fused)
        lg = torch.from_numpy(p["logit"])
        for b in range(3):
            a = torch.softmax(lg[b, :p["n_live"][b]], dim=0)           # float64: exp(-200) is not 0 there, but 1e-87
            assert np.array_equal(a.argmax(0).numpy(), p["tstar"][b]) and float((1 - a.max(0).values).max()) < 1e-80
            assert np.float32(np.exp(np.float32(-200.0))) == 0.0
        assert np.array_equal(np.take_along_axis(p["h"], p["tstar"][:, None, :], 1)[:, 0], p["mean"])
        assert {0, 1, 3, 4, 63, 64, 127, 200} <= set(p["tstar"][1].tolist()) and (p["h"][0, 128:] == E.POISON).all()
        a1, wc = E.attend_factors(p["logit"])
        assert np.array_equal(np.einsum("btk,ck->btc", a1, wc), p["logit"]) and set(a1.sum(2).ravel()) == {1.0}
    u = E.pool_uniform_case(3, 128, 128)
    assert np.array_equal(u["h"].mean(1), u["mean"]) and (u["logit"] == u["logit"][:, :1]).all()


def test_argmax_reference_is_numpy_argmax():
    for N_, K, D in ((1, 1, 7), (41, 5, 192), (130, 64, 200)):
        w, c, best, score = E.argmax_case(N_, K, D)
        sim = w.astype(np.float32) @ c.astype(np.float32).T
        assert np.array_equal(np.argmax(sim, axis=1), best) and np.array_equal(sim.max(1), score.astype(np.float32))
        if K >= 5:
            assert np.array_equal(c[0], c[K - 1]) and np.array_equal(c[3], c[4]) and not (best == K - 1).any() and not (best == 4).any()


# ------------------------------------------------------------------ 2. bit budgets

def test_an_oversized_case_is_refused():
    with pytest.raises(E.BudgetError, match="2\\^24"):
        E.oversized_case()
    with pytest.raises(E.BudgetError, match="f16"):                   # a dense case that is fine in f32 leaves the f16 budget
        E.dense_case("oversized-f16", dict(B=1, T=64, cin=4096, cout=64, k=3, dil=1), f16=True, kernels=())
    with pytest.raises(E.BudgetError, match="power of two"):
        E.colstat_case("C3x128-256", 3, 96, 256)
    with pytest.raises(E.BudgetError):
        E.need_mean("thirds", np.array([1.0]), 3)
    with pytest.raises(KeyError):
        E.register("no-such-case")


def test_every_conv_case_states_its_budget():
    for name in E.CONV_CASE_NAMES:
        c = E.conv_case(name)
        assert 0 < c.bound < E.F32_LIMIT and np.abs(c.y).max() < E.F32_LIMIT
        for a in (c.x, c.w, c.y) if c.f16 else ():
            assert np.abs(a).max() <= E.F16_LIMIT and np.array_equal(a.astype(np.float16).astype(np.float64), a)
        if c.kind.startswith("split"):
            big = c.x if c.kind == "split_x" else c.w
            assert set(np.unique(big)) == {-2049.0, 0.0, 2049.0}


# ------------------------------------------------------------------ 3. coverage

# every kernel the exact tests are held to, stated here a second time: a name dropped from the helper's table fails below
CONV_KERNELS = ("conv_gemm_f32_kernel", "conv_gemm_f32_s64_kernel", "skinny_gemm_f32_kernel", "conv_gemm_f32_vh_kernel", "conv_gemm_f32_n64_kernel",
                "conv_gemm_f32_t256_kernel", "conv_gemm_f32_packed_kernel", "seg_gemm_partial_f32_kernel", "seg_gemm_reduce_f32_kernel",
                "conv_gemm_f16_kernel", "conv_gemm_f16_t256_kernel", "conv_gemm_split16_n128_kernel",
                "split16_pack_kernel", "res2net_chain_f16_kernel", "chain_pack_kernel")
FAMILIES = {
    "segment statistics": ("seg_mean_std_kernel", "se_scale_residual_kernel", "colstat_finish_kernel"),
    "pooling": ("asp_pool_kernel", "asp_pool_lds_kernel"),
    "fused pooling": ("asp_attend_pool_f32_kernel", "asp_attend_pool_f16_kernel"),
    "affinity": ("affinity_sym_kernel", "l2norm_rows_kernel", "adjacent_cosine_kernel", "fill_f32_kernel"),
    "ahc": ("ahc_nearest_kernel", "ahc_nearest_finish_kernel", "ahc_merge_kernel"),
    "spectral": ("affinity_apply_kernel", "apply_finish_kernel", "affinity_degree_kernel"),
    "sim_argmax": ("sim_argmax_kernel",), "topk": ("topk_mean_std_kernel",), "viterbi": ("viterbi_kernel",),
}
# every LABEL they are held to: what the census (kernel_census.KERNEL_TESTS) sends to tests/test_gpu_exact.py
EXACT_LABELS = {lb for lb, t in kernel_census.KERNEL_TESTS.items() if t and t[0] == "test_gpu_exact"}


def _coverage_gaps(table):
    """Kernels without a gather and a dense case, families without both kinds, and labels without any case."""
    cov = E.coverage(table)
    by_kernel = {}
    for lb, names in cov.items():
        by_kernel.setdefault(E.kernel_of(lb), set()).update(names)
    kinds = lambda k: {table[n][0] for n in by_kernel.get(k, ())}  # noqa: E731
    gaps = [k for k in CONV_KERNELS if kinds(k) != {"gather", "dense"}]
    # the wide split form shares its kernel with the f16 operator: its labels need a gather and a dense case of their own
    split = {table[n][0] for lb, names in cov.items() if lb.startswith("conv_gemm_f16_t256_kernel<split,") for n in names}
    gaps += ["conv_gemm_f16_t256_kernel<split>"] if split != {"gather", "dense"} else []
    for fam, kernels in FAMILIES.items():
        gaps += [k for k in kernels if not by_kernel.get(k)]
        if set().union(*(kinds(k) for k in kernels)) != {"gather", "dense"}:
            gaps.append(fam)
    return gaps + sorted(lb for lb in EXACT_LABELS if not cov.get(lb) and lb not in gaps)


def test_exact_coverage_names_a_gather_and_a_dense_case_for_every_kernel():
    """... and, since the launch log, a case for every launch label the census sends to tests/test_gpu_exact.py."""
    assert E.EXACT_COVERAGE == E.coverage() and _coverage_gaps(E.CASE_TABLE) == []
    assert set(E.EXACT_COVERAGE) == EXACT_LABELS
    assert {E.kernel_of(lb) for lb in EXACT_LABELS} == set(CONV_KERNELS) | {k for ks in FAMILIES.values() for k in ks} == set(E.ALL_KERNELS)
    assert set(E.CONV_CASE_NAMES) == {n for n in E.CASE_TABLE if E.CASE_TABLE[n][1] and n.split("-")[0] in tuple(E.SHAPES) or n[0] == "C"}
    # the check bites: without its packed cases, or without the one-hot chain, the table has a gap
    without = lambda pred: _coverage_gaps({n: v for n, v in E.CASE_TABLE.items() if not pred(n)})  # noqa: E731
    assert without(lambda n: n.startswith("P-")) == ["conv_gemm_f32_packed_kernel"]
    assert without(lambda n: n == "chain-onehot") == ["res2net_chain_f16_kernel", "chain_pack_kernel"]
    assert "viterbi_kernel" in without(lambda n: n.startswith("viterbi"))
    # ... and over labels: the 64-row ring kernel is reached by S5 alone, the lockstep walk of the wide split form by W1024 alone, the
    # symmetric band walk of the 128x128 kernel by the affinity of 1412 rows alone
    assert without(lambda n: n.startswith("S5-")) == ["conv_gemm_f32_s64_kernel<64>"]
    assert without(lambda n: n.startswith("W1024-")) == ["conv_gemm_f16_t256_kernel<split,direct>/lockstep"]
    assert without(lambda n: n[0] == "W" and n.endswith(("-rows", "-chan"))) == ["split16_pack_kernel", "conv_gemm_f16_t256_kernel<split>"]
    assert "conv_gemm_f32_kernel<dma>/symmetric" in without(lambda n: n == "affinity-k16")


def test_the_f32_label_table_is_the_dispatch_rule_restated():
    """F32_LABELS (data, derived by hand beside each entry) against kernel_selection.f32_conv_label (sd_choose_conv_f32 restated as
    code): two statements of the same rules must agree on every shape and selection."""
    for shape, by_sel in E.F32_LABELS.items():
        assert list(by_sel) == kernel_selection.CONV_KERNELS
        if shape[0] == "C":
            (B, T), cout = (int(v) for v in shape[1:].split("-")[0].split("x")), int(shape.split("-")[1])
        else:
            B, T, cout = (E.SHAPES[shape][k] for k in ("B", "T", "cout"))
        for sel, label in by_sel.items():
            assert kernel_selection.f32_conv_label(sel, B * T, T, cout, colstat=shape[0] == "C") == label, (shape, sel)
    # the pins fall through exactly where a side condition fails
    assert kernel_selection.f32_conv_label("rows96", 70, 1, 40) == "conv_gemm_f32_kernel<dma>"                  # T == 1
    assert kernel_selection.f32_conv_label("wide256", 262, 131, 1016) == "conv_gemm_f32_kernel<dma>"            # cout < 1024
    assert kernel_selection.f32_conv_label("wide256", 704, 64, 1024, colstat=True) == "conv_gemm_f32_kernel<dma>"     # colstat at T < 128


def test_every_kernel_of_the_table_exists_in_the_sources():
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "speech-diarization_amd", "csrc")
    text = "".join(open(os.path.join(root, f)).read() for f in sorted(os.listdir(root)) if f.endswith(".hip"))
    for k in E.ALL_KERNELS:
        assert f" {k}(" in text, k


# ------------------------------------------------------------------ 4. the expected values are reachable in the kernels' arithmetic

@pytest.mark.parametrize("name", [n for n in E.CONV_CASE_NAMES if E.CASE_TABLE[n][0] == "dense"])
def test_dense_cases_are_exact_in_torch_f32(name):
    """The same conv and epilogue in f32 on the CPU (another summation order again) gives the integer answer bit for bit."""
    c = E.conv_case(name)
    y, tee = _conv1d_ref(c, torch.float32)
    assert torch.equal(y, torch.from_numpy(c.y).float()) and torch.equal(y.double(), torch.from_numpy(c.y))
    if c.tee_hi:
        assert torch.equal(tee, torch.from_numpy(c.tee).float())
    if c.f16:
        assert torch.equal(y.half().float(), y) and (not c.tee_hi or torch.equal(tee.half().float(), tee))


@pytest.mark.parametrize("name", [n for n in E.CONV_CASE_NAMES if "split_" in n])
def test_split16_decomposition_and_three_products_are_exact(name):
    """hi = f16(v), lo = f16(v - hi): 2049 s -> (2048 s, s) exactly; with the weights pre-scaled by 2^s as the pack does,
    hi.hi + hi.lo + lo.hi summed in f32, times 2^-s, is the integer sum, and lo.lo is zero."""
    from speech_diarization_amd.engine import pack_conv_weight_split16
    c = E.conv_case(name)
    assert np.float16(2049.0) == 2048.0 and np.float16(2049.0 - 2048.0) == 1.0
    x = torch.from_numpy(c.x).float()
    xh = x.half().float()
    xl = (x - xh).half().float()
    assert torch.equal(xh + xl, x)
    packed, s = pack_conv_weight_split16(c.w.astype(np.float32))
    cp = packed.shape[2] * 32
    wh = torch.from_numpy(packed[..., :32].reshape(c.cout, c.k, cp)[:, :, :c.cin].astype(np.float32))
    wl = torch.from_numpy(packed[..., 32:].reshape(c.cout, c.k, cp)[:, :, :c.cin].astype(np.float32))
    assert torch.equal((wh + wl) * 2.0 ** -s, torch.from_numpy(c.w).float().permute(0, 2, 1))
    if c.kind == "split_x":
        assert bool(xl.any()) and not bool(wl.any())
    else:
        assert bool(wl.any()) and not bool(xl.any())
    src = torch.from_numpy(E.source_rows(c.lengths, c.k, c.dil))
    acc = torch.zeros(c.M, c.cout)
    for j in range(c.k):
        for a, b in ((xh, wh), (xh, wl), (xl, wh)):
            acc = acc + a[src[:, j]] @ b[:, j].T
    want = torch.from_numpy(E.conv_sum(c.x, c.w, src.numpy())).float()
    assert torch.equal(acc * 2.0 ** -s, want)
    y = acc * 2.0 ** -s
    if c.bias is not None:
        b = torch.from_numpy(c.bias).float()
        y = y + (torch.repeat_interleave(b, torch.tensor(c.lengths), dim=0) if c.bias_per_seg else b)
    y = (torch.relu(y) if c.act == "relu" else y) * torch.from_numpy(c.scale).float() + torch.from_numpy(c.shift).float()
    assert torch.equal(y, torch.from_numpy(c.y).float())
