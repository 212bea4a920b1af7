"""The grouped HDBSCAN route on the GPU: `sd_hdb_core_grouped_f32` and `sd_hdb_outgoing_grouped_f32` (include/sd_hip_hdbscan.h) bit for
bit against `sd_hdb_core_f32` and `sd_hdb_outgoing_f32` on every group alone, exactly against their numpy statement on integer rows,
the group and component mask, the two promises about `group`, guard bands at exact buffer sizes, `hdbscan_gpu.hdbscan_rows_groups`
against `hdbscan_rows` per recording, and `diarize_many` against `diarize` per recording."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import captured as CAP  # noqa: E402
import guarded as G  # noqa: E402
import hdbscan_grouped_ref as HG  # noqa: E402
import hdbscan_ref as H  # noqa: E402
from launch_log import expect_launches, launches  # noqa: E402

pytestmark = pytest.mark.gpu

GRID_D = (192, 190, 7)
KS = (1, 2, 3, 5, 16)
# 49 groups over 1 497 rows: 1, 2, 3, 127, 128, 129 and 300 rows, forty groups of 3 inside tile 5 and 6, two that straddle tile edges.
# No boundary falls on a tile edge by itself (they are 1, 3, 6, 133, 261, 390, 690, 693, ..., 810, 1260)
SIZES = (1, 2, 3, 127, 128, 129, 300) + (3,) * 40 + (450, 237)
# 50 groups over 1 496 rows: boundaries at 128, 256, 384 and 512 exactly, the forty groups of 3 inside tile 1 (rows 128 .. 247)
SIZES_ALIGNED = (128,) + (3,) * 40 + (8, 127, 1, 128, 129, 300, 2, 3, 450, 100)
OUT_LABELS = ["hdb_outgoing_grouped_kernel", "hdb_outgoing_grouped_finish_kernel"]
INF = float("inf")


def _labels(k):
    """The instantiation of the grouped core kernel and of its finish kernel for k neighbours: a running top-1, 2, 4, 8 or 16."""
    kk = next(c for c in (1, 2, 4, 8, 16) if k <= c)
    return [f"hdb_core_grouped_kernel<{kk}>", f"hdb_core_grouped_finish_kernel<{kk}>"]


def _lds(d):
    ld = (d + 3) // 4 * 4
    return ld, ld + 4


def _bits(t):
    return t.contiguous().view(torch.int32)


def _f32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def _unit_case(n, d, ld, seed):
    """f32 [n][ld]: unit rows in columns [0, d), NaN in [d, ld)."""
    S = np.full((n, ld), np.nan, np.float32)
    S[:, :d] = H.unit_rows(np.random.default_rng(seed).standard_normal((n, d)))
    return S


def _bounds(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(int)


def _core_alone(ops, Sv, sizes, k):
    """`ops.hdb_core` on every group's slice; -inf for a group of at most k rows (the ungrouped entry refuses k > n - 1)."""
    out = []
    b = _bounds(sizes)
    for a, e in zip(b[:-1], b[1:]):
        out.append(ops.hdb_core(Sv[a:e], k) if e - a > k else torch.full((e - a,), -INF, device=Sv.device))
    return torch.cat(out)


def _outgoing_alone(ops, Sv, core, comp, sizes):
    """`ops.hdb_outgoing` on every group's slice -> (nn as indices into all rows, -1 kept; best)."""
    nn, best = [], []
    b = _bounds(sizes)
    for a, e in zip(b[:-1], b[1:]):
        g_nn, g_best = ops.hdb_outgoing(Sv[a:e], core[a:e].contiguous(), comp[a:e].contiguous())
        nn.append(torch.where(g_nn >= 0, g_nn + int(a), g_nn))
        best.append(g_best)
    return torch.cat(nn), torch.cat(best)


def _next_components(comp, nn, best):
    """One Boruvka round of `hdbscan_gpu.spanning_edges_groups` on the host: the components after the chosen edges."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from speech_diarization_amd import hdbscan_gpu as hg
    lo, hi, _ = hg._component_edges(comp, nn, best, np.flatnonzero(nn >= 0))
    m = int(comp.max()) + 1
    _, merged = connected_components(coo_matrix((np.ones(lo.size, np.int8), (comp[lo], comp[hi])), shape=(m, m)), directed=False)
    return hg._by_lowest_member(merged[comp])


# ------------------------------------------------------------------ bit for bit against the ungrouped kernels

@pytest.mark.parametrize("sizes", [SIZES, SIZES_ALIGNED], ids=["as_cut", "tile_aligned"])
def test_core_and_outgoing_equal_the_ungrouped_kernels_on_every_group(dev, sizes):
    """For every group: `core` is that of `ops.hdb_core` on the group's slice at every k of KS (every instantiation
    hdb_core_grouped_kernel<KK> and hdb_core_grouped_finish_kernel<KK>, KK = 1, 2, 4, 8, 16, runs and is named by the launch log), -inf
    where the group has at most k rows; nn - offset and the bits of best are those of `ops.hdb_outgoing` on the slice, with core = +inf
    and with the k = 1 core values, at the components of three stages of a real Boruvka run (singletons, after one round, after two).
    The outgoing call runs exactly hdb_outgoing_grouped_kernel and hdb_outgoing_grouped_finish_kernel."""
    from speech_diarization_amd import ops
    n = sum(sizes)
    assert 1450 <= n <= 1550 and 45 <= len(sizes) <= 55 and {1, 2, 3, 127, 128, 129, 300} <= set(sizes) and sizes.count(3) >= 40
    b = _bounds(sizes)
    group = _i32(HG.group_of(sizes), dev)
    max_group = max(sizes)
    for d in GRID_D:
        for ld in _lds(d):
            S = _unit_case(n, d, ld, seed=1000 * n + d)
            Sv = torch.from_numpy(S).to(dev)[:, :d]
            cores = {}
            for k in KS:
                with expect_launches(exactly=_labels(k)):
                    core, bad = ops.hdb_core_grouped(Sv, k, group, max_group)
                core2, _ = ops.hdb_core_grouped(Sv, k, group, max_group)
                want = _core_alone(ops, Sv, sizes, k)
                assert int(bad) == 0 and torch.equal(_bits(core), _bits(core2)), (d, ld, k)                 # bitwise run to run
                assert not bool(torch.isnan(core).any()), "the NaN of columns [d, ld) was read"
                assert torch.equal(_bits(core), _bits(want)), f"d={d} ld={ld} k={k}: {int((_bits(core) != _bits(want)).sum())} core values differ"
                small = np.repeat(np.asarray(sizes) <= k, sizes)
                assert small.any() and bool((core.cpu()[torch.from_numpy(small)] == -INF).all()) and bool(torch.isfinite(core.cpu()[torch.from_numpy(~small)]).all())
                cores[k] = core
            for cname, core in (("inf", torch.full((n,), INF, device=dev)), ("k1", cores[1])):
                comp = np.arange(n, dtype=np.int64)
                for stage in range(3):
                    compd = _i32(comp, dev)
                    with expect_launches(exactly=OUT_LABELS):
                        nn, best, bad = ops.hdb_outgoing_grouped(Sv, core, compd, group, max_group)
                    w_nn, w_best = _outgoing_alone(ops, Sv, core, compd, sizes)
                    assert int(bad) == 0 and not bool(torch.isnan(best).any())
                    assert torch.equal(nn, w_nn), f"d={d} ld={ld} core={cname} stage={stage}: {int((nn != w_nn).sum())} neighbours differ"
                    assert torch.equal(_bits(best), _bits(w_best)), f"d={d} ld={ld} core={cname} stage={stage}: weights differ in their bits"
                    nn_h, best_h = nn.cpu().numpy(), best.cpu().numpy()
                    has = nn_h >= 0
                    assert np.array_equal(HG.group_of(sizes)[nn_h[has]], HG.group_of(sizes)[has]) and (comp[nn_h[has]] != comp[has]).all()
                    if stage == 0:
                        alone = b[:-1][np.asarray(sizes) == 1]
                        assert has.sum() == n - len(alone) and np.all(nn_h[alone] == -1) and np.all(best_h[alone] == -np.inf)
                    comp = _next_components(comp, nn_h, best_h)
                assert len(set(comp.tolist())) < n // 4                                                     # the run went somewhere


# ------------------------------------------------------------------ exact answers

@pytest.mark.parametrize("sizes", [SIZES, SIZES_ALIGNED], ids=["as_cut", "tile_aligned"])
def test_both_entries_equal_the_numpy_statement_on_integer_rows(dev, sizes):
    """Small-integer rows (`hdbscan_ref.integer_rows`): no product and no partial sum rounds, so numpy's f32 Gram is THE answer in any
    summation order, equal scores abound, and the lowest column among equal weights is numpy's argmax.  `torch.equal` only."""
    from speech_diarization_amd import ops
    n = sum(sizes)
    g = HG.group_of(sizes)
    group = _i32(g, dev)
    i = np.arange(n)
    comps = {"singletons": i, "interleaved": i % 2, "tile-aligned": i // 128, "straddling": (i + 64) // 128 * 7 + 3, "one": np.zeros(n, int)}
    for d, ld in ((192, 192), (190, 192), (7, 12)):
        S = H.integer_rows(n, d, ld, seed=300 * n + d)
        Sv = torch.from_numpy(S).to(dev)[:, :d]
        Gm = H.gram_f32(S[:, :d])
        cores = {"inf": np.full(n, np.inf, np.float32)}
        for k in (1, 3, 16):
            core, bad = ops.hdb_core_grouped(Sv, k, group, max(sizes))
            want = HG.core_grouped_from_gram(Gm, k, g).astype(np.float32)
            assert int(bad) == 0 and torch.equal(core, _f32(want, dev)), f"core d={d} k={k}: {int((core.cpu() != torch.from_numpy(want)).sum())} rows differ"
            cores[f"k{k}"] = want
        for cname in ("inf", "k1", "k3"):
            for name, comp in comps.items():
                nn, best, bad = ops.hdb_outgoing_grouped(Sv, _f32(cores[cname], dev), _i32(comp, dev), group, max(sizes))
                w_nn, w_best = HG.outgoing_grouped_from_gram(Gm, cores[cname], comp, g)
                assert int(bad) == 0
                assert torch.equal(nn, _i32(w_nn, dev)), f"nn d={d} core={cname} comp={name}: {int((nn.cpu() != torch.from_numpy(w_nn)).sum())} rows differ"
                assert torch.equal(best, _f32(w_best, dev)), f"best d={d} core={cname} comp={name}"
                if name == "one":
                    assert bool((nn == -1).all()) and bool((best == -INF).all())
        # ties do occur and go to the lowest column: a row whose best weight is attained more than once inside its group
        nn, best, _ = ops.hdb_outgoing_grouped(Sv, _f32(cores["inf"], dev), _i32(i, dev), group, max(sizes))
        W = np.where((g[:, None] == g[None, :]) & (i[:, None] != i[None, :]), Gm, -np.inf)
        tied = ((W == W.max(1, keepdims=True)).sum(1) > 1) & np.isfinite(W.max(1))       # (a row alone in its group has nothing to tie)
        assert tied.sum() > 10 and np.array_equal(nn.cpu().numpy()[tied], W.argmax(1)[tied])


# ------------------------------------------------------------------ the mask

def test_the_mask_keeps_every_edge_inside_its_group_and_out_of_its_component(dev):
    """Copies of one unit row: three in group 0, one in group 1 (the same tile), two in group 3 (tiles 3 and 4 away from the first).
    Their mutual score is the largest there is and the ungrouped kernels take it across the groups; the grouped ones never do.  Then
    two of the copies of group 0 share a component: neither chooses the other, both choose the third."""
    from speech_diarization_amd import ops
    sizes = [60, 60, 300, 100, 80]                                  # groups at rows 0, 60, 120, 420, 520; W = 3 of T - 1 = 4
    n, d = sum(sizes), 192
    X = H.unit_rows(np.random.default_rng(5).standard_normal((n, d)))
    copies = [3, 10, 40, 70, 430, 500]
    X[copies] = X[3]
    Xd, group = torch.from_numpy(X).to(dev), _i32(HG.group_of(sizes), dev)
    g = HG.group_of(sizes)
    inf = torch.full((n,), INF, device=dev)
    comp = np.arange(n)
    nn, best, bad = ops.hdb_outgoing_grouped(Xd, inf, _i32(comp, dev), group, max(sizes))
    nn, best = nn.cpu().numpy(), best.cpu().numpy()
    assert int(bad) == 0 and np.array_equal(g[nn], g)
    assert nn[3] == 10 and nn[10] == 3 and nn[40] == 3 and nn[430] == 500 and nn[500] == 430
    same = [3, 10, 40, 430, 500]
    assert len(set(best[same].view(np.int32).tolist())) == 1 and abs(float(best[3]) - 1.0) <= 1e-6
    assert 60 <= nn[70] < 120 and best[70] < 0.5                    # the largest score of row 70 lies outside its group and is not taken
    full_nn, full_best = ops.hdb_outgoing(Xd, inf, _i32(comp, dev))  # the test bites: without the mask row 70 and the far copies take row 3
    full_nn = full_nn.cpu().numpy()
    assert full_nn[70] == 3 and full_nn[430] == 3 and full_nn[500] == 3 and float(full_best[70]) == float(best[3])
    # the core values: a copy's nearest is another copy only inside its group
    core, bad = ops.hdb_core_grouped(Xd, 1, group, max(sizes))
    core = core.cpu().numpy()
    assert int(bad) == 0 and len(set(core[same].view(np.int32).tolist())) == 1 and core[70] < 0.5 and core[3] == best[3]
    assert float(ops.hdb_core(Xd, 1)[70]) == float(core[3])
    # components inside one group: rows 3 and 10 in one component, row 40 in another
    comp2 = comp.copy()
    comp2[10] = comp2[3]
    comp2[431:520] = comp2[430]                                       # and all of group 3 but row 430's copy partner side: 430 .. 519 one component
    nn2, best2, bad = ops.hdb_outgoing_grouped(Xd, inf, _i32(comp2, dev), group, max(sizes))
    nn2, best2 = nn2.cpu().numpy(), best2.cpu().numpy()
    assert int(bad) == 0 and nn2[3] == 40 and nn2[10] == 40 and nn2[40] == 3 and best2[3] == best[3]
    assert 420 <= nn2[430] < 430 and 420 <= nn2[500] < 430 and best2[430] < 0.5          # the copy at 500 is in 430's component now
    assert np.array_equal(g[nn2], g) and (comp2[nn2] != comp2).all()
    whole = comp.copy()
    whole[60:120] = 60                                                # group 1 is one component: its rows have no edge, every other row keeps its own
    nn3, best3, _ = ops.hdb_outgoing_grouped(Xd, inf, _i32(whole, dev), group, max(sizes))
    nn3, best3 = nn3.cpu().numpy(), best3.cpu().numpy()
    assert (nn3[60:120] == -1).all() and (best3[60:120] == -np.inf).all()
    rest = np.r_[0:60, 120:n]
    assert np.array_equal(nn3[rest], nn[rest]) and np.array_equal(best3[rest].view(np.int32), best[rest].view(np.int32))


# ------------------------------------------------------------------ the promise

def test_a_broken_promise_is_reported(dev):
    """`bad` of both entries is non-zero when a group has more rows than max_group or `group` decreases somewhere, and 0 at the exact
    bound; with one group over everything and max_group = n the entries are `ops.hdb_core` and `ops.hdb_outgoing`, bit for bit."""
    from speech_diarization_amd import ops
    sizes = [5, 300, 129, 40]
    n, d = sum(sizes), 190
    Sv = torch.from_numpy(_unit_case(n, d, 192, seed=9)).to(dev)[:, :d]
    group = _i32(HG.group_of(sizes), dev)
    inf, comp = torch.full((n,), INF, device=dev), _i32(np.arange(n), dev)

    def bads(grp, max_group):
        return int(ops.hdb_core_grouped(Sv, 2, grp, max_group)[1]), int(ops.hdb_outgoing_grouped(Sv, inf, comp, grp, max_group)[2])
    assert bads(group, 300) == (0, 0) and bads(group, 301) == (0, 0) and bads(group, 10 ** 9) == (0, 0)
    for max_group in (299, 1):                                                                 # one below the largest group; far below
        c, o = bads(group, max_group)
        assert c != 0 and o != 0, max_group
    for at, value in ((150, 0), (n - 1, 2), (1, -4)):                                          # one descent: in the middle, at the end, at the start
        down = group.clone()
        down[at] = value
        c, o = bads(down, 300)
        assert HG.promise_broken(down.cpu().numpy(), 300) and c != 0 and o != 0, at
    assert bads(group, 300) == (0, 0)                                                          # `bad` is set to 0 first, every call
    for m in (1, 129, 700):
        Sv = torch.from_numpy(_unit_case(m, d, 192, seed=m)).to(dev)[:, :d]
        zero, compm = torch.zeros(m, dtype=torch.int32, device=dev), _i32(np.arange(m) // 3, dev)
        nn, best, bad = ops.hdb_outgoing_grouped(Sv, torch.full((m,), INF, device=dev), compm, zero, m)
        want_nn, want_best = ops.hdb_outgoing(Sv, torch.full((m,), INF, device=dev), compm)
        assert int(bad) == 0 and torch.equal(nn, want_nn) and torch.equal(_bits(best), _bits(want_best)), m
        if m > 3:
            core, bad = ops.hdb_core_grouped(Sv, 3, zero, m)
            assert int(bad) == 0 and torch.equal(_bits(core), _bits(ops.hdb_core(Sv, 3))), m


# ------------------------------------------------------------------ exact buffer sizes, guard bands (style of tests/test_gpu_ahc_grouped.py)

EDGE_SHAPES = [(1, 4, 4, 1, 1), (5, 7, 8, 2, 1), (129, 190, 192, 129, 16), (257, 192, 192, 3, 2), (1000, 192, 196, 300, 5)]      # (n, d, ld, max_group, k)


@pytest.mark.parametrize("n,d,ld,max_group,k", EDGE_SHAPES)
def test_entries_at_exact_buffer_sizes(dev, n, d, ld, max_group, k):
    """Every buffer ends at its last element (the last row of `rows` at column d), both workspaces have exactly the bytes of their
    formula: one byte less is refused, nothing outside is written, the NaN of the padding columns [d, ld) is never read, and the
    results are those of the wrapper's own allocations.  Then the two broken promises (a decreasing `group`, a group above max_group)
    on the same buffers: `bad` is set and every guard band is still intact, whatever `group` holds."""
    from speech_diarization_amd import _native as N, ops
    lib = N.load()
    sizes = [max_group] * (n // max_group) + ([n % max_group] if n % max_group else [])
    S = _unit_case(n, d, ld, seed=n + d)
    Sv = torch.from_numpy(S).to(dev)[:, :d]
    group_h = HG.group_of(sizes)
    comp_h = (np.arange(n) // 2).astype(np.int32)
    groupd, compd = _i32(group_h, dev), _i32(comp_h, dev)
    want_core, want_bad = ops.hdb_core_grouped(Sv, k, groupd, max_group)
    core_in = torch.where(torch.isfinite(want_core), want_core, torch.full_like(want_core, INF))
    want_nn, want_best, want_bad2 = ops.hdb_outgoing_grouped(Sv, core_in, compd, groupd, max_group)
    assert int(want_bad) == 0 == int(want_bad2) and not bool(torch.isnan(want_best).any()) and not bool(torch.isnan(want_core).any())
    flat = torch.from_numpy(S.reshape(-1)[: (n - 1) * ld + d].copy())
    need_c = int(lib.sd_hdb_core_grouped_workspace_bytes(n, d, k, max_group))
    need_o = int(lib.sd_hdb_outgoing_grouped_workspace_bytes(n, d, max_group))
    assert need_c == HG.core_workspace_bytes(n, k, max_group) and need_o == HG.outgoing_workspace_bytes(n, max_group)
    broken = []
    if n > 1:
        down = group_h.copy()
        down[n // 2] = down.max() + 5                                  # a descent after row n / 2, values far outside [0, groups)
        down[0] = -(2 ** 31)
        broken.append((down, max_group))
        broken.append((np.zeros(n, np.int32), max(1, n // 2)))        # one group of n rows above max_group = n / 2
        broken.append((np.full(n, 2 ** 31 - 1, np.int32), 1))
    for poison in G.POISONS:
        for grp, mg in [(group_h, max_group)] + broken:
            good = grp is group_h
            nc, no = int(lib.sd_hdb_core_grouped_workspace_bytes(n, d, k, mg)), int(lib.sd_hdb_outgoing_grouped_workspace_bytes(n, d, mg))
            gS = G.guarded_from(flat, dev, "rows")
            gg = G.guarded_from(torch.from_numpy(grp), dev, "group")
            gc = G.guarded(n * 4, poison, dev, "core")
            gbad = G.guarded(4, poison, dev, "bad")
            gw = G.guarded(nc, poison, dev, "core ws")
            args = (gS.ptr, ld, n, d, k, gg.ptr, mg, gc.ptr, gbad.ptr, gw.ptr)
            assert CAP.call("sd_hdb_core_grouped_f32", *args, nc - 1) == -3                      # one byte short
            N.check(CAP.call("sd_hdb_core_grouped_f32", *args, nc), "sd_hdb_core_grouped_f32")
            torch.cuda.synchronize()
            G.assert_guards_intact(gS, gg, gc, gbad, gw)
            assert (int(gbad.view(torch.int32)[0]) == 0) == good, (poison, mg)
            if good:
                assert nc == need_c and torch.equal(_bits(gc.view(torch.float32)), _bits(want_core)), poison
            gci = G.guarded_from(core_in.cpu(), dev, "core in")
            gcomp = G.guarded_from(torch.from_numpy(comp_h), dev, "comp")
            gn, gb, gbad2 = G.guarded(n * 4, poison, dev, "nn"), G.guarded(n * 4, poison, dev, "best"), G.guarded(4, poison, dev, "bad")
            gwo = G.guarded(no, poison, dev, "outgoing ws")
            args = (gS.ptr, ld, n, d, gci.ptr, gcomp.ptr, gg.ptr, mg, gn.ptr, gb.ptr, gbad2.ptr, gwo.ptr)
            assert CAP.call("sd_hdb_outgoing_grouped_f32", *args, no - 1) == -3
            N.check(CAP.call("sd_hdb_outgoing_grouped_f32", *args, no), "sd_hdb_outgoing_grouped_f32")
            torch.cuda.synchronize()
            G.assert_guards_intact(gS, gg, gci, gcomp, gn, gb, gbad2, gwo)
            assert (int(gbad2.view(torch.int32)[0]) == 0) == good, (poison, mg)
            if good:
                assert no == need_o and torch.equal(gn.view(torch.int32), want_nn) and torch.equal(_bits(gb.view(torch.float32)), _bits(want_best)), poison


def test_lib_refuses_on_the_device_too(dev):
    """Refusals of tests/test_hdbscan_grouped_rules.py with real device buffers: nothing is written, `bad` included."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    S = torch.ones((64, 192), device=dev)
    group, comp = torch.zeros(64, dtype=torch.int32, device=dev), torch.arange(64, dtype=torch.int32, device=dev)
    core, best = torch.full((64,), 7.0, device=dev), torch.full((64,), 7.0, device=dev)
    nn, bad = torch.full((64,), 7, dtype=torch.int32, device=dev), torch.full((1,), 7, dtype=torch.int32, device=dev)
    ws = torch.empty(max(int(lib.sd_hdb_core_grouped_workspace_bytes(64, 192, 2, 64)), int(lib.sd_hdb_outgoing_grouped_workspace_bytes(64, 192, 64))),
                     dtype=torch.uint8, device=dev)

    def c(rows=S.data_ptr(), ld=192, n=64, d=192, k=2, max_group=64, ws_bytes=ws.numel()):
        return CAP.call("sd_hdb_core_grouped_f32", rows, ld, n, d, k, group.data_ptr(), max_group, core.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws_bytes)

    def o(rows=S.data_ptr(), ld=192, n=64, d=192, max_group=64, ws_bytes=ws.numel()):
        return lib.sd_hdb_outgoing_grouped_f32(rows, ld, n, d, core.data_ptr(), comp.data_ptr(), group.data_ptr(), max_group, nn.data_ptr(),
                                               best.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws_bytes, None)
    assert c(ld=190, d=190) == -1 and c(rows=S.data_ptr() + 4, n=63) == -1 and c(max_group=0) == -1 and c(k=0) == -1 and c(k=17) == -2 and c(ws_bytes=15) == -3
    assert o(ld=190, d=190) == -1 and o(rows=S.data_ptr() + 4, n=63) == -1 and o(max_group=0) == -1 and o(ws_bytes=15) == -3
    torch.cuda.synchronize()
    assert bool((nn == 7).all()) and bool((best == 7.0).all()) and bool((core == 7.0).all()) and int(bad) == 7
    assert c() == 0
    torch.cuda.synchronize()
    assert bool((core == 192.0).all()) and int(bad) == 0
    bad.fill_(7)
    assert o() == 0
    torch.cuda.synchronize()
    assert float(best[5]) == 192.0 and int(nn[0]) == 1 and int(nn[5]) == 0 and int(bad) == 0


# ------------------------------------------------------------------ the driver

def test_driver_on_a_folder_of_65_recordings(dev):
    """64 recordings of 300 planted rows (different seeds) and one of 3 001 in one driver: the labels of every recording equal
    `hdbscan_rows` on it alone, exactly (the arithmetic is the same bits and the edge lists are the same arrays: this needs no
    condition on ties), and the rounds are the maximum of the recordings' rounds.

    The three counts of the first (core) pass over the 22 201 rows, T = 174 tiles a side: a full walk of the Gram is 174^2 = 30 276
    tiles; the recordings' own squares, were each aligned to a tile edge, are 64 x 3^2 + 24^2 = 1 152; the band walk computes the tiles
    a recording actually reaches, fewer than twice that (a 300-row recording that starts inside a tile touches 4 tile rows, not 3)."""
    from speech_diarization_amd import hdbscan_gpu
    parts = [H.planted(300, 3, 0.5, 100 + s, 0) for s in range(64)]
    parts.insert(10, H.planted(3001, 6, 0.8, 99, 30))
    sizes = [len(x) for x in parts]
    b = _bounds(sizes)
    Xd = torch.from_numpy(np.concatenate(parts)).to(dev)
    labels, info = hdbscan_gpu.hdbscan_rows_groups(Xd, sizes, return_info=True)
    rounds = []
    for i, (a, e, got) in enumerate(zip(b[:-1], b[1:], labels)):
        want, inf = hdbscan_gpu.hdbscan_rows(Xd[a:e], return_info=True)
        assert np.array_equal(got, want), (i, int((got != want).sum()))
        assert info["mst_weight"][i] == inf["mst_weight"]
        rounds.append(inf["rounds"])
    full, squares = (-(-sum(sizes) // 128)) ** 2, sum((-(-m // 128)) ** 2 for m in sizes)
    first = info["gram_tiles_per_pass"][0]
    print(f"{len(sizes)} recordings, {sum(sizes)} rows: rounds alone max {max(rounds)} sum {sum(rounds)}, together {info['rounds']}; "
          f"first pass {first} tiles, the recordings' squares {squares}, a full walk {full}; all passes {info['gram_tiles']}")
    assert info["rounds"] == max(rounds) <= 12 and (full, squares) == (30276, 1152)
    assert squares <= first < 2 * squares and first * 10 < full
    assert len(info["gram_tiles_per_pass"]) == 1 + info["rounds"] and info["gram_tiles"] == sum(info["gram_tiles_per_pass"])
    again = hdbscan_gpu.hdbscan_rows_groups(Xd, sizes)
    assert all(np.array_equal(p, q) for p, q in zip(labels, again))
    # another setting, with noise labels: diar_diag's (6, 3, False)
    labels = hdbscan_gpu.hdbscan_rows_groups(Xd[: b[12]], sizes[:12], 6, 3, False)
    for a, e, got in zip(b[:12], b[1:13], labels):
        assert np.array_equal(got, hdbscan_gpu.hdbscan_rows(Xd[a:e], 6, 3, False))
    assert any((lab < 0).any() for lab in labels)


def test_driver_refuses_before_a_launch(dev):
    from speech_diarization_amd import hdbscan_gpu
    X = torch.from_numpy(np.concatenate([H.planted(100, 2, 0.5, 0, 0), H.planted(300, 3, 0.5, 1, 0)])).to(dev)
    Xb = X.clone()
    Xb[117, 3] = float("nan")
    with launches() as log:
        with pytest.raises(ValueError, match="recording 1: rows must be finite"):
            hdbscan_gpu.hdbscan_rows_groups(Xb, [100, 300])
        with pytest.raises(ValueError, match="recording 0: metric 'euclidean' takes unit rows"):
            hdbscan_gpu.hdbscan_rows_groups(X * 2.0, [100, 300])
        with pytest.raises(ValueError, match="recording 1: min_samples"):
            hdbscan_gpu.hdbscan_rows_groups(X, [100, 3, 297], 2, 4)
        assert [lab.tolist() for lab in hdbscan_gpu.hdbscan_rows_groups(X[:2], [1, 0, 1])] == [[0], [], [0]]
    assert log == {}


# ------------------------------------------------------------------ the pipeline

@pytest.fixture()
def small_encoder(dev):
    """The small seeded encoder of tests/test_gpu_hdbscan.py."""
    from speech_diarization_amd import ecapa_annote, speech_encode, synth
    enc = speech_encode.HipEcapaEncoder(synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(128)), dev)
    speech_encode.using_ecapa_encoder.cache_clear()
    orig = speech_encode.using_ecapa_encoder
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = lambda device="cuda": enc
    yield enc
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = orig


def test_diarize_many_equals_diarize_per_recording(small_encoder):
    """Two conversations, a silent recording and one with a single segment: `diarize_many` gives the segments of
    `diarize(..., clusterer="hdbscan_gpu")` on each, segment for segment.  The embeddings are computed per recording in both routes (the
    same launches), so the clusterers see the same rows and the equality needs no margin."""
    from speech_diarization_amd import anti_stick_diarize as asd, synth
    conv_a, conv_b = synth.synthetic_conversation(24.0, 2, seed=0), synth.synthetic_conversation(20.0, 3, seed=5)
    first = asd.diarize(conv_a.wav, 16000, scd_thr=1.5, clusterer="hdbscan_gpu")
    a0 = int(first[0].start * 16000)
    waves = [conv_a.wav, np.zeros(3 * 16000, np.float32), conv_b.wav, conv_a.wav[a0:a0 + int(1.2 * 16000)].copy()]
    want = [asd.diarize(w, 16000, scd_thr=1.5, clusterer="hdbscan_gpu") for w in waves]
    with launches() as log:
        got = asd.diarize_many(waves, 16000, scd_thr=1.5)
    assert len(got) == 4
    for w, g in zip(want, got):
        assert [(s.start, s.end, s.spk) for s in g] == [(s.start, s.end, s.spk) for s in w]
    print(f"segments {[len(g) for g in got]}, speakers {[len({s.spk for s in g}) for g in got]}")
    # (the seeded, untrained encoder tells no voices apart: what the tail leaves is one speaker per recording, here as in `diarize`)
    assert len(got[0]) >= 1 and got[1] == [] and len(got[2]) >= 2 and len(got[3]) == 1
    assert log.get("hdb_outgoing_grouped_kernel", 0) >= 1 and "hdb_outgoing_kernel" not in log          # the folder went through the grouped driver
