"""The device AHC route on the GPU: the two entries of include/sd_hip_ahc.h against f64 / the numpy statement over a shape grid,
run-to-run reproducibility, guard bands at exact buffer sizes, and `ahc_gpu` against `cluster.ahc_cosine` end to end."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import ahc_ref as A  # noqa: E402
import captured as CAP  # noqa: E402
import guarded as G  # noqa: E402
import spectral_ref as R  # noqa: E402
from launch_log import expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu

GRID_N = (1, 2, 5, 127, 128, 129, 257, 1000, 3001)
GRID_D = (192, 190, 7)


def _lds(d):
    ld = (d + 3) // 4 * 4
    return ld, ld + 4


def _bits(t):
    return t.contiguous().view(torch.int32)


def _on(dev, S, d, count, inv):
    """The [n][ld] matrix with its NaN padding on the device and the view of its first d columns the wrappers take."""
    Sd = torch.from_numpy(S).to(dev)
    return Sd, Sd[:, :d], torch.from_numpy(count).to(dev), torch.from_numpy(inv).to(dev)


# ------------------------------------------------------------------ nearest

@pytest.mark.parametrize("n", GRID_N)
def test_nearest_against_f64(dev, n):
    """|best - best64| <= (d + 4) 2^-23 (|a| |b|) inv_i inv_j: the f32 dot-product bound d 2^-24 |a| |b| with 2 x slack, the three
    roundings of the scale included.  The index is the f64 argmax wherever the f64 top two are more than two bounds apart, and within
    a bound of the maximum elsewhere (ahc_ref.check_nearest)."""
    from speech_diarization_amd import ops
    for d in GRID_D:
        for ld in _lds(d):
            S, count, inv = A.grid_case(n, d, ld, seed=1000 * n + d)
            _, Sv, _, invd = _on(dev, S, d, count, inv)
            nn, best = ops.ahc_nearest(Sv, invd)
            nn2, best2 = ops.ahc_nearest(Sv, invd)
            assert torch.equal(nn, nn2) and torch.equal(_bits(best), _bits(best2))               # bitwise run to run
            nn, best = nn.cpu().numpy(), best.cpu().numpy()
            assert not np.isnan(best).any(), "the NaN of columns [d, ld) was read"
            worst = A.check_nearest(nn, best, S[:, :d], inv, d)
            print(f"nearest n={n} d={d} ld={ld}: error / bound {worst:.4f}")
            if n > 1:                                                                          # reciprocal pairs carry the same bits
                mutual = nn[nn] == np.arange(n)
                assert mutual.any()
                assert np.array_equal(best[mutual].view(np.int32), best[nn[mutual]].view(np.int32))


def test_nearest_duplicated_rows_choose_the_lowest_index(dev):
    """Copies of one unit row in three different tiles: their mutual score is the largest there is, bitwise the same in every tile
    and in both triangles, and every row reports the lowest index that attains it."""
    from speech_diarization_amd import ops
    n, d = 300, 192
    X = A.unit_rows(np.random.default_rng(5).standard_normal((n, d)))
    copies = [3, 10, 131, 200, 290]
    X[copies] = X[3]
    nn, best = ops.ahc_nearest(torch.from_numpy(X).to(dev), torch.ones(n, device=dev))
    nn, best = nn.cpu().numpy(), best.cpu().numpy()
    assert nn[3] == 10 and all(nn[c] == 3 for c in copies[1:])
    assert len(set(best[copies].view(np.int32).tolist())) == 1 and abs(float(best[3]) - 1.0) <= 1e-6
    # a tie among columns that are no copies of the row: rows 50 and 180 are the same, so every other row scores them equally
    X2 = A.unit_rows(np.random.default_rng(6).standard_normal((n, d)))
    X2[180] = X2[50]
    nn2, _ = ops.ahc_nearest(torch.from_numpy(X2).to(dev), torch.ones(n, device=dev))
    nn2 = nn2.cpu().numpy()
    assert nn2[50] == 180 and nn2[180] == 50 and not (np.delete(nn2, 50) == 180).any()


# ------------------------------------------------------------------ merge

@pytest.mark.parametrize("n", [2, 129, 1000])
def test_merge_equals_the_numpy_statement_bit_for_bit(dev, n):
    from speech_diarization_amd import ops
    for d, ld in ((192, 192), (190, 196), (7, 8)):
        S, count, inv = A.grid_case(n, d, ld, seed=77 * n + d)
        Sd, Sv, _, invd = _on(dev, S, d, count, inv)
        with expect_launches(exactly=["ahc_nearest_kernel", "ahc_nearest_finish_kernel"]):
            nn, best = ops.ahc_nearest(Sv, invd)
        nn_h, best_h = nn.cpu().numpy(), best.cpu().numpy()
        # thresholds: below every score (every reciprocal pair merges), the median best of the reciprocal pairs (some do), above
        # every score (none does)
        mid = float(np.median(best_h[nn_h[nn_h] == np.arange(n)]))
        for thr in (-1e30, mid, 1e30):
            Sd, Sv, countd, invd = _on(dev, S, d, count, inv)
            with expect_launches(exactly=["ahc_merge_kernel"]):
                target, merged = ops.ahc_merge(Sv, countd, invd, nn, best, thr)
            w_s, w_c, w_i, w_t, w_m = A.merge_f32(S[:, :d], count, inv, nn_h, best_h, thr)
            assert int(merged) == w_m and np.array_equal(target.cpu().numpy(), w_t)
            assert np.array_equal(Sd[:, :d].cpu().numpy().view(np.int32), w_s.view(np.int32))
            assert np.array_equal(Sd[:, d:].cpu().numpy().view(np.int32), S[:, d:].view(np.int32))   # the padding keeps its bytes
            assert np.array_equal(countd.cpu().numpy().view(np.int32), w_c.view(np.int32))
            assert np.array_equal(invd.cpu().numpy().view(np.int32), w_i.view(np.int32))
            print(f"merge n={n} d={d} ld={ld} thr={thr:.3g}: {w_m} pairs")
            if thr == -1e30:
                assert w_m >= 1
            if thr == 1e30:
                assert w_m == 0
        if n >= 129:
            assert 0 < A.merge_f32(S[:, :d], count, inv, nn_h, best_h, mid)[4] < A.merge_f32(S[:, :d], count, inv, nn_h, best_h, -1e30)[4]


# ------------------------------------------------------------------ exact buffer sizes, guard bands (style of test_gpu_buffer_edges.py)

EDGE_SHAPES = [(1, 4, 4), (1, 7, 8), (5, 7, 8), (129, 190, 192), (129, 192, 192), (257, 190, 196), (1000, 192, 196)]      # (n, d, ld)


@pytest.mark.parametrize("n,d,ld", EDGE_SHAPES)
def test_both_entries_at_exact_buffer_sizes(dev, n, d, ld):
    """Every buffer ends at its last element (the last row of `sums` at column d), the workspace has exactly the bytes the formula
    gives: nothing outside is written, and the results are those of the wrappers' own allocations."""
    from speech_diarization_amd import _native as N, ops
    lib = N.load()
    S, count, inv = A.grid_case(n, d, ld, seed=n + d)
    _, Sv, countd, invd = _on(dev, S, d, count, inv)
    want_nn, want_best = ops.ahc_nearest(Sv, invd)
    mutual = want_nn.cpu().numpy()[want_nn.cpu().numpy()] == np.arange(n) if n > 1 else np.zeros(1, bool)
    thr = float(np.median(want_best.cpu().numpy()[mutual])) if n > 1 else 0.0                # some reciprocal pairs merge, some do not
    flat = torch.from_numpy(S.reshape(-1)[: (n - 1) * ld + d].copy())
    need = int(lib.sd_ahc_nearest_workspace_bytes(n, d))
    for poison in G.POISONS:
        gS = G.guarded_from(flat, dev, "sums")
        gi = G.guarded_from(torch.from_numpy(inv), dev, "inv_count")
        gc = G.guarded_from(torch.from_numpy(count), dev, "count")
        gn, gb = G.guarded(n * 4, poison, dev, "nn"), G.guarded(n * 4, poison, dev, "best")
        gw = G.guarded(need, poison, dev, "ws")
        assert CAP.call("sd_ahc_nearest_f32", gS.ptr, ld, n, d, gi.ptr, gn.ptr, gb.ptr, gw.ptr, need - 1) == -3        # one byte short
        N.check(CAP.call("sd_ahc_nearest_f32", gS.ptr, ld, n, d, gi.ptr, gn.ptr, gb.ptr, gw.ptr, need), "sd_ahc_nearest_f32")
        torch.cuda.synchronize()
        G.assert_guards_intact(gS, gi, gn, gb, gw)
        assert torch.equal(gn.view(torch.int32), want_nn) and torch.equal(_bits(gb.view(torch.float32)), _bits(want_best)), poison
        gt, gm = G.guarded(n * 4, poison, dev, "target"), G.guarded(4, poison, dev, "n_merged")
        N.check(CAP.call("sd_ahc_merge_f32", gS.ptr, ld, n, d, gc.ptr, gi.ptr, gn.ptr, gb.ptr, thr, gt.ptr, gm.ptr), "sd_ahc_merge_f32")
        torch.cuda.synchronize()
        G.assert_guards_intact(gS, gc, gi, gn, gb, gt, gm)
        w_s, w_c, w_i, w_t, w_m = A.merge_f32(S[:, :d], count, inv, want_nn.cpu().numpy(), want_best.cpu().numpy(), thr)
        assert int(gm.view(torch.int32)[0]) == w_m and np.array_equal(gt.view(torch.int32).cpu().numpy(), w_t)
        got = np.full(n * ld, np.nan, np.float32)
        got[: (n - 1) * ld + d] = gS.view(torch.float32).cpu().numpy()
        assert np.array_equal(got.reshape(n, ld)[:, :d].view(np.int32), w_s.view(np.int32))
        assert np.array_equal(gc.view(torch.float32).cpu().numpy().view(np.int32), w_c.view(np.int32))
        assert np.array_equal(gi.view(torch.float32).cpu().numpy().view(np.int32), w_i.view(np.int32))


def test_lib_refuses_on_the_device_too(dev):
    """Refusals of tests/test_ahc_rules.py with real device buffers: nothing is written."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    S = torch.ones((64, 192), device=dev)
    inv = torch.ones(64, device=dev)
    nn = torch.full((64,), 7, dtype=torch.int32, device=dev)
    best = torch.full((64,), 7.0, device=dev)
    ws = torch.empty(int(lib.sd_ahc_nearest_workspace_bytes(64, 192)), dtype=torch.uint8, device=dev)
    assert CAP.call("sd_ahc_nearest_f32", S.data_ptr(), 190, 64, 190, inv.data_ptr(), nn.data_ptr(), best.data_ptr(), ws.data_ptr(), ws.numel()) == -1
    assert CAP.call("sd_ahc_nearest_f32", S.data_ptr() + 4, 192, 63, 192, inv.data_ptr(), nn.data_ptr(), best.data_ptr(), ws.data_ptr(), ws.numel()) == -1
    assert CAP.call("sd_ahc_nearest_f32", S.data_ptr(), 192, 64, 192, inv.data_ptr(), nn.data_ptr(), best.data_ptr(), ws.data_ptr(), ws.numel() - 1) == -3
    torch.cuda.synchronize()
    assert bool((nn == 7).all()) and bool((best == 7.0).all())
    assert CAP.call("sd_ahc_nearest_f32", S.data_ptr(), 192, 64, 192, inv.data_ptr(), nn.data_ptr(), best.data_ptr(), ws.data_ptr(), ws.numel()) == 0
    torch.cuda.synchronize()
    assert float(best[5]) == 192.0 and int(nn[0]) == 1 and int(nn[5]) == 0


# ------------------------------------------------------------------ the driver

def _same_partition(got, want):
    from speech_diarization_amd import cluster
    return np.array_equal(cluster.relabel_by_first_appearance(got), cluster.relabel_by_first_appearance(want))


@pytest.fixture(scope="module")
def host_side(dev):
    """(rows, device rows, host affinity) per family, formed once: the affinity is what the host route downloads."""
    from speech_diarization_amd import ops
    cache = {}

    def get(rows):
        if rows not in cache:
            X, _ = A.family_rows(rows)
            Xd = torch.from_numpy(X).to(dev)
            cache[rows] = (Xd, ops.cosine_affinity(Xd).cpu().numpy())
        return cache[rows]
    return get


@pytest.mark.parametrize("rows,thr", A.DRIVER_PAIRS)
def test_driver_partition_equals_the_host_route(host_side, rows, thr):
    from speech_diarization_amd import ahc_gpu, cluster
    Xd, K = host_side(rows)
    margin = A.cut_margin(K, thr)
    assert margin > A.CUT_MARGIN, margin
    want = cluster.ahc_cosine(K, thr)
    got, info = ahc_gpu.ahc_cosine_rows(Xd, thr, return_info=True)
    print(f"rows={rows} thr={thr}: cut margin {margin:.2e}, {info['clusters']} clusters, {info['rounds']} rounds, "
          f"gram_rows / N^2 {info['gram_rows'] / rows ** 2:.2f}, last_best {info['last_best']:.4f}")
    assert _same_partition(got, want), f"{int((got != cluster.relabel_by_first_appearance(want)).sum())} of {rows} labels differ"
    assert np.array_equal(got, cluster.relabel_by_first_appearance(got))
    assert info["clusters"] == len(np.unique(want))
    again = ahc_gpu.ahc_cosine_rows(Xd, thr)
    assert np.array_equal(got, again)                                                          # equal labels run to run


@pytest.mark.parametrize("thr", [0.3, 0.05])
def test_driver_duplicate_rows_and_zero_rows(dev, thr):
    from speech_diarization_amd import ahc_gpu, cluster, ops
    X = A.duplicates_and_zero_rows()
    Xd = torch.from_numpy(X).to(dev)
    K = ops.cosine_affinity(Xd).cpu().numpy()
    assert np.all(K[-3:] == 0)
    got = ahc_gpu.ahc_cosine_rows(Xd, thr)
    assert _same_partition(got, cluster.ahc_cosine(K, thr))
    assert np.array_equal(got[300:350], got[:50])


def test_driver_refuses_a_nan_row_and_takes_tiny_inputs(dev):
    from speech_diarization_amd import ahc_gpu
    X = torch.from_numpy(A.family_rows(400)[0]).to(dev)
    X[17, 3] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        ahc_gpu.ahc_cosine_rows(X, 0.3)
    two = torch.tensor([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0]], device=dev)
    assert ahc_gpu.ahc_cosine_rows(two[:0], 0.5).tolist() == [] and ahc_gpu.ahc_cosine_rows(two[:1], 0.5).tolist() == [0]
    assert ahc_gpu.ahc_cosine_rows(two, 0.5).tolist() == [0, 0] and ahc_gpu.ahc_cosine_rows(two, 0.7).tolist() == [0, 1]
    labels, info = ahc_gpu.ahc_cosine_rows(torch.from_numpy(A.family_rows(400)[0]).to(dev), 1.5, return_info=True)
    assert labels.tolist() == list(range(400)) and info["rounds"] == 0 and info["gram_rows"] == 160000


def test_scale_20k_rows_12_planted_speakers(dev):
    """No host reference at this size in test time (a 3.2 GB f64 matrix and scipy's linkage over it): the check is against the
    planted labels."""
    from speech_diarization_amd import ahc_gpu
    n, k = 20000, 12
    X, planted = R.planted_rows(n, k, 0.5, 5, dtype=np.float32)
    labels, info = ahc_gpu.ahc_cosine_rows(torch.from_numpy(X).to(dev), 0.3, return_info=True)
    print(f"N={n}: {info['clusters']} clusters, {info['rounds']} rounds, gram_rows / N^2 {info['gram_rows'] / n ** 2:.2f}, "
          f"last_best {info['last_best']:.4f}")
    assert info["clusters"] == k
    assert _same_partition(labels, planted)


# ------------------------------------------------------------------ the pipeline

def _small_sd(width=128):
    from speech_diarization_amd import synth
    return synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(width))


@pytest.fixture()
def small_encoder(dev):
    from speech_diarization_amd import ecapa_annote, speech_encode
    enc = speech_encode.HipEcapaEncoder(_small_sd(), dev)
    speech_encode.using_ecapa_encoder.cache_clear()
    orig = speech_encode.using_ecapa_encoder
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = lambda device="cuda": enc
    yield enc
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = orig


PIPELINE_THRS = (0.70, 0.95)


@pytest.mark.parametrize("thr", PIPELINE_THRS)
def test_rttm_is_byte_identical_on_the_device_route(small_encoder, tmp_path, thr):
    """The thresholds come from the sweep of tools/sweep_ahc_threshold.py on the MI355X over this meeting (60 s, 2 voices, seed 0, the
    small seeded encoder, 119 windows), cosine -0.5 .. 0.95 in steps of 0.05: the host route finds 2 speakers at every cut up to 0.90
    and 4 at 0.95; the cut margin is 0.234 at 0.70 (the reference's threshold and the default) and 9.3e-3 at 0.95, the smallest of
    the sweep.  Both are asserted again here."""
    from speech_diarization_amd import audio_io, diarization_baseline as db, synth
    conv = synth.synthetic_conversation(60.0, 2, seed=0)
    wav = tmp_path / "meeting.wav"
    audio_io.write_wav16(wav, conv.wav, conv.sr)
    seg_h, det_h = db.diarize_audio(wav, 0.35, 0.1, 2, 6, rttm_filepath=tmp_path / "host.rttm", clustering="ahc", clustering_threshold=thr,
                                    return_details=True)
    speakers = len(set(det_h["labels"].tolist()))
    margin = A.cut_margin(det_h["affinity"], thr)
    print(f"{len(det_h['labels'])} windows at {thr}: {speakers} speakers on the host route, cut margin {margin:.2e}")
    assert 2 <= speakers <= 8 and margin > A.CUT_MARGIN
    seg_d, det_d = db.diarize_audio(wav, 0.35, 0.1, 2, 6, rttm_filepath=tmp_path / "dev.rttm", clustering="ahc_gpu", clustering_threshold=thr,
                                    return_details=True)
    assert (tmp_path / "dev.rttm").read_bytes() == (tmp_path / "host.rttm").read_bytes()
    assert seg_d == seg_h and np.array_equal(det_d["labels"], det_h["labels"])
    assert det_d["affinity"] is None                                                           # no affinity is formed on this route
    hp = db.DiarizationParameters(min_speakers=2, max_speakers=6, clustering_threshold=thr)
    assert db.Diarizer(hp, clustering="ahc_gpu").diarize(wav, None) == db.Diarizer(hp, clustering="ahc").diarize(wav, None)


def test_clusterer_through_the_two_stage_glue(dev):
    """No embedding involved: `AhcGpuClusterer` where the glue takes a `clusterer_factory`, against `cluster.AhcClusterer`.  The
    two-stage glue hands its clusterers rows (metric "euclidean"); the single-stage one hands over a distance matrix, which the device
    route refuses."""
    from speech_diarization_amd import ahc_gpu, cluster
    X, _ = A.family_rows(400)
    got = cluster.cluster_hdbscan_two_stage(X, clusterer_factory=ahc_gpu.AhcGpuClusterer.factory(0.3))
    want = cluster.cluster_hdbscan_two_stage(X, clusterer_factory=cluster.AhcClusterer.factory(0.3))
    assert _same_partition(got, want) and len(set(got.tolist())) >= 2
    with pytest.raises(ValueError, match="precomputed"):
        cluster.cluster_hdbscan(X, clusterer_factory=ahc_gpu.AhcGpuClusterer.factory(0.3))
