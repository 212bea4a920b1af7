"""The device HDBSCAN route on the GPU: the two entries of include/sd_hip_hdbscan.h against their numpy statement on exact (integer)
inputs with `torch.equal`, the bitwise identities the header promises (both entries see the same products, w is symmetric, runs
repeat), guard bands at exact buffer sizes, the f32 bound against float64, and `hdbscan_gpu` against scikit-learn's HDBSCAN end to
end."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import captured as CAP  # noqa: E402
import guarded as G  # noqa: E402
import hdbscan_ref as H  # noqa: E402
from launch_log import expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu

EXACT_N = (2, 3, 127, 128, 129, 257, 300)
EXACT_D = (4, 190, 192)
LD = 192
INF = float("inf")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ks(n):
    """k on both edges of every instantiation of the core kernel (a running top-1, 2, 4, 8 or 16): 1, 2, 3-4, 5-8, 9-16."""
    return sorted({k for k in (1, 2, 3, 4, 5, 8, 9, 16, n - 1) if 1 <= k <= min(16, n - 1)})


def _core_labels(k):
    """The instantiation of the core kernel and of its finish kernel for k neighbours: a running top-1, 2, 4, 8 or 16."""
    kk = next(c for c in (1, 2, 4, 8, 16) if k <= c)
    return [f"hdb_core_kernel<{kk}>", f"hdb_core_finish_kernel<{kk}>"]


def _components(n):
    """name -> comp int32 [n]: singletons, two interleaved, aligned to the 128-row tile edge, straddling it, one component."""
    i = np.arange(n)
    return {"singletons": i, "interleaved": i % 2, "tile-aligned": i // 128, "straddling": (i + 64) // 128 * 7 + 3, "three-way": (i * 7) % 3,
            "one": np.zeros(n, int)}


def _f32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


# ------------------------------------------------------------------ exact: torch.equal only

@pytest.mark.parametrize("n", EXACT_N)
def test_core_equals_the_numpy_kth_largest_on_integer_rows(dev, n):
    """Small-integer rows: every product and partial sum is an integer far below 2^24, so numpy's f32 Gram is THE answer in any
    summation order, and equal scores abound (duplicates count).  Columns [d, 192) hold NaN and are never read."""
    from speech_diarization_amd import ops
    for d in EXACT_D:
        S = H.integer_rows(n, d, LD, seed=100 * n + d)
        Sd = torch.from_numpy(S).to(dev)
        Gm = H.gram_f32(S[:, :d])
        for k in _ks(n):
            with expect_launches(exactly=_core_labels(k)):
                got = ops.hdb_core(Sd[:, :d], k)
            want = torch.from_numpy(H.core_from_gram(Gm, k).astype(np.float32)).to(dev)
            assert torch.equal(got, want), f"core n={n} d={d} k={k}: {int((got != want).sum())} rows differ"


@pytest.mark.parametrize("n", EXACT_N)
def test_outgoing_equals_the_numpy_statement_on_integer_rows(dev, n):
    from speech_diarization_amd import ops
    for d in EXACT_D:
        S = H.integer_rows(n, d, LD, seed=200 * n + d)
        Sd = torch.from_numpy(S).to(dev)
        Gm = H.gram_f32(S[:, :d])
        cores = {"inf": np.full(n, np.inf, np.float32)}
        if n > 2:
            cores["k2"] = H.core_from_gram(Gm, 2).astype(np.float32)
        for cname, core in cores.items():
            for name, comp in _components(n).items():
                with expect_launches(exactly=["hdb_outgoing_kernel", "hdb_outgoing_finish_kernel"]):
                    nn, best = ops.hdb_outgoing(Sd[:, :d], _f32(core, dev), _i32(comp, dev))
                w_nn, w_best = H.outgoing_from_gram(Gm, core, comp)
                assert torch.equal(nn, _i32(w_nn, dev)), f"nn n={n} d={d} core={cname} comp={name}: {int((nn.cpu() != torch.from_numpy(w_nn)).sum())} rows differ"
                assert torch.equal(best, _f32(w_best, dev)), f"best n={n} d={d} core={cname} comp={name}"
                if name == "one":
                    assert bool((nn == -1).all()) and bool((best == -INF).all())


TIED = (15, 16, 63, 64, 127, 128, 129, 200, 255, 256)        # lane (16), wave (64) and tile (128) boundaries


def _tied_rows(n=300, d=192):
    """Every row is e_0 plus -1 / 0 / 1 in three more columns; the TIED rows are all 5 e_0.  So every row scores exactly 5 against
    every TIED column and at most 4 against any other, and a TIED row scores 25 against the other TIED ones."""
    rng = np.random.default_rng(9)
    S = np.zeros((n, d), np.float32)
    S[:, 0] = 1.0
    S[:, 1:4] = rng.integers(-1, 2, (n, 3))
    S[list(TIED)] = 0.0
    S[list(TIED), 0] = 5.0
    return S


@pytest.mark.parametrize("cut", TIED)
def test_the_lowest_of_tied_columns_wins_on_both_sides_of_the_diagonal(dev, cut):
    """The TIED columns below `cut` share one component with every ordinary row, so an ordinary row's closest rows are all in its own
    component and must be skipped; the lowest column left to it is `cut`, left of the diagonal for the rows past it, right of it for
    the rows before it."""
    from speech_diarization_amd import ops
    S = _tied_rows()
    n = S.shape[0]
    Gm = H.gram_f32(S)
    comp = np.arange(n) + 1
    comp[[t for t in range(n) if t not in TIED]] = 0
    comp[[t for t in TIED if t < cut]] = 0
    ordinary = np.array([i for i in range(n) if i not in TIED])
    for cname, core in (("inf", np.full(n, np.inf, np.float32)), ("k16", H.core_from_gram(Gm, 16).astype(np.float32))):
        nn, best = ops.hdb_outgoing(_f32(S, dev), _f32(core, dev), _i32(comp, dev))
        w_nn, w_best = H.outgoing_from_gram(Gm, core, comp)
        assert torch.equal(nn, _i32(w_nn, dev)) and torch.equal(best, _f32(w_best, dev)), (cut, cname)
        nn = nn.cpu().numpy()
        assert (nn[ordinary] == cut).all(), (cut, cname)
        later = [t for t in TIED if t > cut]
        if later:
            assert nn[cut] == (TIED[0] if cut > TIED[0] else later[0]) and all(nn[t] == TIED[0] if cut > TIED[0] else nn[t] == cut for t in later)
    assert (ordinary < cut).any() and (ordinary > cut).any()
    # the multiset rule of the core entry on the same rows: ten columns tie at 5, so the 1st .. 10th largest of an ordinary row are all 5
    for k in (1, 2, 10, 11):
        got = ops.hdb_core(_f32(S, dev), k)
        assert torch.equal(got, _f32(H.core_from_gram(Gm, k), dev))
        assert bool((got[torch.from_numpy(ordinary).to(dev)] == 5.0).all()) == (k <= 10)


# ------------------------------------------------------------------ the identities of the header

@pytest.mark.parametrize("n", [300, 700])
def test_both_entries_see_the_same_bits_and_w_is_symmetric(dev, n):
    from speech_diarization_amd import ops
    X = _f32(H.unit_rows(np.random.default_rng(n).standard_normal((n, 190))), dev)
    Xp = torch.nn.functional.pad(X, (0, 2), value=float("nan"))[:, :190]               # ld = 192, d = 190
    singles = torch.arange(n, dtype=torch.int32, device=dev)
    inf = torch.full((n,), INF, device=dev)
    core1 = ops.hdb_core(Xp, 1)
    nn, best = ops.hdb_outgoing(Xp, inf, singles)
    assert torch.equal(_bits(best), _bits(core1)), "the two entries round the same pair differently"
    for k in (2, 5):
        core = ops.hdb_core(Xp, k)
        assert torch.equal(_bits(core), _bits(ops.hdb_core(Xp, k)))                    # run to run
        assert bool((core <= core1).all()) and bool((core < core1).any())
        for comp in (singles, singles // 3, (singles * 5) % 7):
            nn, best = ops.hdb_outgoing(Xp, core, comp.contiguous())
            nn2, best2 = ops.hdb_outgoing(Xp, core, comp.contiguous())
            assert torch.equal(nn, nn2) and torch.equal(_bits(best), _bits(best2))      # run to run
            nn_l = nn.long()
            assert bool((nn_l >= 0).all()) and bool((comp[nn_l] != comp).all())
            mutual = nn_l[nn_l] == torch.arange(n, device=dev)
            assert bool(mutual.any())
            assert torch.equal(_bits(best[mutual]), _bits(best[nn_l[mutual]])), "w(i, j) != w(j, i)"


@pytest.mark.parametrize("n", [300, 700])
def test_against_float64(dev, n):
    """|core - core64| and |best - best64| <= (d + 4) 2^-23 |a| |b| (hdbscan_ref.dot_bound: the f32 dot-product bound with 2 x slack;
    the k-th largest, min and max are 1-Lipschitz in the max norm, so the bound on a product is the bound on either result)."""
    from speech_diarization_amd import ops
    d = 192
    Xh = H.unit_rows(np.random.default_rng(7 * n).standard_normal((n, d)))
    bound = float(H.dot_bound(Xh, d).max())
    X = _f32(Xh, dev)
    comp = np.arange(n) // 5
    for k in (1, 2, 16):
        core = ops.hdb_core(X, k)
        core64, W64 = H.reach_f64(Xh, k)
        e_core = float(np.abs(core.cpu().numpy().astype(np.float64) - core64).max())
        nn, best = ops.hdb_outgoing(X, core, _i32(comp, dev))
        W64[comp[:, None] == comp[None, :]] = -np.inf
        e_best = float(np.abs(best.cpu().numpy().astype(np.float64) - W64.max(1)).max())
        nn = nn.cpu().numpy()
        e_own = float(np.abs(best.cpu().numpy().astype(np.float64) - W64[np.arange(n), nn]).max())
        print(f"n={n} k={k}: core error {e_core:.2e}, best error {e_best:.2e}, bound {bound:.2e}")
        assert e_core <= bound and e_best <= bound and e_own <= bound


TWIN_SHAPES = [(2, 1, 4), (129, 33, 36), (300, 192, 192)]      # (n, d, ld)


@pytest.mark.parametrize("n,d,ld", TWIN_SHAPES)
def test_outgoing_without_core_and_components_is_the_nearest_pass_of_ahc(dev, n, d, ld):
    """The two files compute with one tile (csrc/sd_gram_tile.h): with core = +inf and every row a component of its own,
    w = fminf(+inf, acc) = acc and every other row is a candidate; with inv_count = 1 the AHC score is acc · (1 · 1) = acc.  Both
    sides are exact, so `nn` and the bits of `best` must agree.  (129, 33, 36) puts one row into the second row and column block,
    ends d inside a group of four and pads the stride; 300 rows have diagonal, off-diagonal and partial tiles.  Rows of -2 .. 2 tie
    everywhere (the lowest-index rule); unit rows round."""
    from speech_diarization_amd import ops
    ints = H.integer_rows(n, d, ld, seed=300 * n + d, lo=-2, hi=3)
    unit = np.full((n, ld), np.nan, np.float32)
    unit[:, :d] = H.unit_rows(np.random.default_rng(n + d).standard_normal((n, d)))
    inf = torch.full((n,), INF, device=dev)
    singles = torch.arange(n, dtype=torch.int32, device=dev)
    ones = torch.ones((n,), device=dev)
    for name, S in (("integer", ints), ("unit", unit)):
        Sv = torch.from_numpy(S).to(dev)[:, :d]
        with expect_launches(exactly=["hdb_outgoing_kernel", "hdb_outgoing_finish_kernel"]):
            nn_h, best_h = ops.hdb_outgoing(Sv, inf, singles)
        with expect_launches(exactly=["ahc_nearest_kernel", "ahc_nearest_finish_kernel"]):
            nn_a, best_a = ops.ahc_nearest(Sv, ones)
        assert torch.equal(nn_h, nn_a), f"nn {name} rows: {int((nn_h != nn_a).sum())} of {n} differ"
        assert torch.equal(_bits(best_h), _bits(best_a)), f"best {name} rows: {int((_bits(best_h) != _bits(best_a)).sum())} of {n} differ"
        assert bool((nn_h >= 0).all()) and bool((nn_h != singles).all())


# ------------------------------------------------------------------ exact buffer sizes, guard bands

EDGE_SHAPES = [(2, 4, 4), (3, 7, 8), (129, 190, 192), (300, 192, 192), (257, 190, 196)]      # (n, d, ld)


@pytest.mark.parametrize("n,d,ld", EDGE_SHAPES)
def test_both_entries_at_exact_buffer_sizes(dev, n, d, ld):
    """Every buffer ends at its last element (the last row of `rows` at column d), each workspace has exactly the bytes its formula
    gives: nothing outside is written, one byte less is refused, and the results are those of the wrappers' own allocations."""
    from speech_diarization_amd import _native as N, ops
    lib = N.load()
    S = H.integer_rows(n, d, ld, seed=n + d)
    k = min(2, n - 1)
    comp = (np.arange(n) // 3).astype(np.int32)
    Sv = torch.from_numpy(S).to(dev)[:, :d]
    want_core = ops.hdb_core(Sv, k)
    want_nn, want_best = ops.hdb_outgoing(Sv, want_core, _i32(comp, dev))
    flat = torch.from_numpy(S.reshape(-1)[: (n - 1) * ld + d].copy())
    need_c, need_o = int(lib.sd_hdb_core_workspace_bytes(n, d, k)), int(lib.sd_hdb_outgoing_workspace_bytes(n, d))
    assert need_c > 0 and need_o > 0
    for poison in G.POISONS:
        gS = G.guarded_from(flat, dev, "rows")
        gc, gw = G.guarded(n * 4, poison, dev, "core"), G.guarded(need_c, poison, dev, "core ws")
        assert CAP.call("sd_hdb_core_f32", gS.ptr, ld, n, d, k, gc.ptr, gw.ptr, need_c - 1) == -3                    # one byte short
        N.check(CAP.call("sd_hdb_core_f32", gS.ptr, ld, n, d, k, gc.ptr, gw.ptr, need_c), "sd_hdb_core_f32")
        torch.cuda.synchronize()
        G.assert_guards_intact(gS, gc, gw)
        assert torch.equal(_bits(gc.view(torch.float32)), _bits(want_core)), poison
        gp = G.guarded_from(torch.from_numpy(comp), dev, "comp")
        gn, gb = G.guarded(n * 4, poison, dev, "nn"), G.guarded(n * 4, poison, dev, "best")
        go = G.guarded(need_o, poison, dev, "outgoing ws")
        assert CAP.call("sd_hdb_outgoing_f32", gS.ptr, ld, n, d, gc.ptr, gp.ptr, gn.ptr, gb.ptr, go.ptr, need_o - 1) == -3
        N.check(CAP.call("sd_hdb_outgoing_f32", gS.ptr, ld, n, d, gc.ptr, gp.ptr, gn.ptr, gb.ptr, go.ptr, need_o), "sd_hdb_outgoing_f32")
        torch.cuda.synchronize()
        G.assert_guards_intact(gS, gc, gp, gn, gb, go)
        assert torch.equal(gn.view(torch.int32), want_nn) and torch.equal(_bits(gb.view(torch.float32)), _bits(want_best)), poison


def test_lib_refuses_on_the_device_too(dev):
    """Refusals of tests/test_hdbscan_rules.py with real device buffers: nothing is written."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    S = torch.ones((64, 192), device=dev)
    core = torch.full((64,), 7.0, device=dev)
    comp = torch.arange(64, dtype=torch.int32, device=dev)
    nn = torch.full((64,), 7, dtype=torch.int32, device=dev)
    best = torch.full((64,), 7.0, device=dev)
    need = int(lib.sd_hdb_outgoing_workspace_bytes(64, 192))
    ws = torch.empty(max(need, int(lib.sd_hdb_core_workspace_bytes(64, 192, 16))), dtype=torch.uint8, device=dev)
    assert CAP.call("sd_hdb_core_f32", S.data_ptr(), 192, 64, 192, 17, core.data_ptr(), ws.data_ptr(), ws.numel()) == -2
    assert CAP.call("sd_hdb_core_f32", S.data_ptr(), 192, 64, 192, 64, core.data_ptr(), ws.data_ptr(), ws.numel()) == -2
    assert CAP.call("sd_hdb_core_f32", S.data_ptr(), 192, 10, 192, 10, core.data_ptr(), ws.data_ptr(), ws.numel()) == -1
    assert CAP.call("sd_hdb_core_f32", S.data_ptr(), 190, 64, 190, 2, core.data_ptr(), ws.data_ptr(), ws.numel()) == -1
    assert CAP.call("sd_hdb_core_f32", S.data_ptr(), 192, 64, 192, 2, core.data_ptr(), ws.data_ptr(), 0) == -3
    assert CAP.call("sd_hdb_outgoing_f32", S.data_ptr() + 4, 192, 63, 192, core.data_ptr(), comp.data_ptr(), nn.data_ptr(), best.data_ptr(), ws.data_ptr(), ws.numel()) == -1
    assert CAP.call("sd_hdb_outgoing_f32", S.data_ptr(), 192, 64, 192, core.data_ptr(), comp.data_ptr(), nn.data_ptr(), best.data_ptr(), ws.data_ptr(), need - 1) == -3
    torch.cuda.synchronize()
    assert bool((nn == 7).all()) and bool((best == 7.0).all()) and bool((core == 7.0).all())
    assert CAP.call("sd_hdb_outgoing_f32", S.data_ptr(), 192, 64, 192, core.data_ptr(), comp.data_ptr(), nn.data_ptr(), best.data_ptr(), ws.data_ptr(), ws.numel()) == 0
    assert CAP.call("sd_hdb_core_f32", S.data_ptr(), 192, 64, 192, 3, core.data_ptr(), ws.data_ptr(), ws.numel()) == 0
    torch.cuda.synchronize()
    assert float(best[5]) == 7.0 and int(nn[0]) == 1 and int(nn[5]) == 0 and float(core[9]) == 192.0


# ------------------------------------------------------------------ the driver

@pytest.fixture(scope="module")
def rows_of():
    cache = {}

    def get(shape, seed):
        if (shape, seed) not in cache:
            cache[shape, seed] = H.planted(shape[0], shape[1], shape[2], seed, shape[3])
        return cache[shape, seed]
    return get


DEVICE_LABEL_CASES = [c for c in H.LABEL_CASES if c[0][0] <= 1000] + [c for c in H.LABEL_CASES if c[0][0] == 2000][:1]


@pytest.mark.parametrize("shape,setting,seed", DEVICE_LABEL_CASES)
def test_labels_equal_scikit_learns(dev, rows_of, shape, setting, seed):
    """Same partition and same noise set as sklearn.cluster.HDBSCAN on the host, for "euclidean" on the rows and for "precomputed"
    1 - cos against the route's "cosine" (the table of tests/test_hdbscan_rules.py up to N = 1000, and one case of 2000 rows)."""
    from speech_diarization_amd import hdbscan_gpu
    X = rows_of(shape, seed)
    Xd = torch.from_numpy(X).to(dev)
    got_e, info = hdbscan_gpu.hdbscan_rows(Xd, *setting, metric="euclidean", return_info=True)
    got_c = hdbscan_gpu.hdbscan_rows(Xd, *setting, metric="cosine")
    print(f"{shape} {setting} seed {seed}: {info['rounds']} rounds {info['components_per_round']}, mst weight {info['mst_weight']:.4f}")
    assert np.array_equal(got_e, hdbscan_gpu.hdbscan_rows(Xd, *setting, metric="euclidean"))      # equal labels run to run
    assert H.same_clustering(got_e, H.host_labels(X, setting, "euclidean")), "euclidean"
    assert H.same_clustering(got_c, H.host_labels(X, setting, "precomputed")), "cosine against precomputed"


def test_driver_argument_rules_on_the_device(dev):
    from speech_diarization_amd import hdbscan_gpu
    X = torch.from_numpy(H.planted(300, 4, 0.6, 0, 0)).to(dev)
    assert hdbscan_gpu.hdbscan_rows(X[:0]).tolist() == [] and hdbscan_gpu.hdbscan_rows(X[:1]).tolist() == [0]
    assert hdbscan_gpu.hdbscan_rows(X[:2]).tolist() == [0, 0]
    with pytest.raises(ValueError, match="min_samples"):
        hdbscan_gpu.hdbscan_rows(X[:10], 2, 11)
    with pytest.raises(ValueError, match="unit rows"):
        hdbscan_gpu.hdbscan_rows(X * 2.0)
    bad = X.clone()
    bad[17, 3] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        hdbscan_gpu.hdbscan_rows(bad)
    got, info = hdbscan_gpu.hdbscan_rows(X, 5, 1, return_info=True)                       # min_samples 1: no core pass
    assert info["gram_rows"] == info["rounds"] * 300 * 300
    assert H.same_clustering(got, H.host_labels(X.cpu().numpy(), (5, 1, True), "euclidean"))
    got = hdbscan_gpu.hdbscan_rows(X[:, :190] * 3.0, 5, None, metric="cosine")           # 190 columns: padded to 192
    assert H.same_clustering(got, H.host_labels(X[:, :190].cpu().numpy(), (5, None, True), "precomputed"))


def test_clusterer_through_the_glue(dev, rows_of):
    """`HdbscanGpuClusterer.factory()` where the two-stage glue takes a `clusterer_factory`, against the default factory; the
    single-stage route `cluster_hdbscan(use_gpu="rows")` against the host's."""
    from speech_diarization_amd import anti_stick_diarize as asd, cluster, hdbscan_gpu
    for shape, seed in (((1000, 8, 0.8, 20), 0), ((700, 3, 0.5, 0), 1)):
        X = rows_of(shape, seed) * np.float32(3.0)
        got = cluster.cluster_hdbscan_two_stage(X, 2, clusterer_factory=hdbscan_gpu.HdbscanGpuClusterer.factory())
        want = cluster.cluster_hdbscan_two_stage(X, 2)
        assert H.same_clustering(got, want) and 0 < int((want < 0).sum()) < len(want)
        assert H.same_clustering(asd.cluster_hdbscan(X, 2, use_gpu="rows"), asd.cluster_hdbscan(X, 2, use_gpu=False))
    with pytest.raises(ValueError, match="precomputed"):
        cluster.cluster_hdbscan(rows_of((700, 3, 0.5, 0), 1), clusterer_factory=hdbscan_gpu.HdbscanGpuClusterer.factory())


# ------------------------------------------------------------------ the pipeline

@pytest.fixture()
def small_encoder(dev):
    from speech_diarization_amd import ecapa_annote, speech_encode, synth
    enc = speech_encode.HipEcapaEncoder(synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(128)), dev)
    speech_encode.using_ecapa_encoder.cache_clear()
    orig = speech_encode.using_ecapa_encoder
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = lambda device="cuda": enc
    yield enc
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = orig


def test_diarize_gives_the_default_clusterers_segments(small_encoder):
    from speech_diarization_amd import anti_stick_diarize as asd, synth
    conv = synth.synthetic_conversation(40.0, 3, seed=5)
    want = asd.diarize(conv.wav, 16000, scd_thr=1.5)
    got = asd.diarize(conv.wav, 16000, scd_thr=1.5, clusterer="hdbscan_gpu")
    print(f"{len(want)} segments, {len({s.spk for s in want})} speakers")
    assert want and [(s.start, s.end, s.spk) for s in got] == [(s.start, s.end, s.spk) for s in want]
