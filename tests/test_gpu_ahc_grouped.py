"""The grouped AHC route on the GPU: `sd_ahc_nearest_grouped_f32` (include/sd_hip_ahc.h) bit for bit against `sd_ahc_nearest_f32` on
every group alone and against f64, the group mask, the two promises about `group`, guard bands at exact buffer sizes,
`ahc_gpu.ahc_cosine_groups` against `ahc_cosine_rows` per recording, a folder-sized case against its planted partitions, and
`diarize_audios` against `diarize_audio` per recording."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import ahc_grouped_ref as AG  # noqa: E402
import ahc_ref as A  # noqa: E402
import captured as CAP  # noqa: E402
import guarded as G  # noqa: E402
import spectral_ref as R  # noqa: E402
from launch_log import expect_launches, launches  # noqa: E402

pytestmark = pytest.mark.gpu

GRID_D = (192, 190, 7)
# the issue's cut: no boundary of it falls on a tile edge by itself (they are 1, 3, 8, 135, 263, 392, 649, 769, 1769), the 257-row and the
# 1000-row groups straddle tile edges
SIZES = (1, 2, 5, 127, 128, 129, 257) + (3,) * 40 + (1000, 1)
# the same sizes in another order: boundaries at 128, 256 and 512 exactly, and the forty groups of 3 inside tile 1 (rows 128 .. 247)
SIZES_ALIGNED = (128,) + (3,) * 40 + (5, 2, 1, 127, 129, 257, 1000, 1)
LABELS = ["ahc_nearest_grouped_kernel", "ahc_nearest_grouped_finish_kernel"]


def _lds(d):
    ld = (d + 3) // 4 * 4
    return ld, ld + 4


def _bits(t):
    return t.contiguous().view(torch.int32)


def _on(dev, S, d, inv):
    """The view of the first d columns of the [n][ld] matrix (NaN padding behind them) on the device, and the reciprocal counts."""
    return torch.from_numpy(S).to(dev)[:, :d], torch.from_numpy(inv).to(dev)


def _group(dev, sizes):
    return torch.from_numpy(AG.group_of(sizes)).to(dev)


def _alone(ops, Sv, invd, sizes):
    """`ops.ahc_nearest` on every group's slice -> (nn as indices into all rows, -1 kept; best), on the host."""
    nn, best = [], []
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    for a, b in zip(bounds[:-1], bounds[1:]):
        g_nn, g_best = ops.ahc_nearest(Sv[a:b], invd[a:b])
        nn.append(torch.where(g_nn >= 0, g_nn + int(a), g_nn))
        best.append(g_best)
    return torch.cat(nn).cpu().numpy(), torch.cat(best).cpu().numpy()


# ------------------------------------------------------------------ nearest

@pytest.mark.parametrize("sizes", [SIZES, SIZES_ALIGNED], ids=["as_cut", "tile_aligned"])
def test_nearest_equals_the_ungrouped_kernel_on_every_group(dev, sizes):
    """For every group, nn - offset and the bits of best are those of `ops.ahc_nearest` on the group's slice (the parent's kernel), and
    the f64 contract of tests/test_gpu_ahc.py holds per group (ahc_ref.check_nearest: |best - best64| <= (d + 4) 2^-23 |a| |b| inv_i
    inv_j).  The call runs exactly ahc_nearest_grouped_kernel and ahc_nearest_grouped_finish_kernel, twice with the same bits."""
    from speech_diarization_amd import ops
    n = sum(sizes)
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    group = _group(dev, sizes)
    for d in GRID_D:
        for ld in _lds(d):
            S, count, inv = A.grid_case(n, d, ld, seed=1000 * n + d)
            Sv, invd = _on(dev, S, d, inv)
            with expect_launches(exactly=LABELS):
                nn, best, bad = ops.ahc_nearest_grouped(Sv, invd, group, max(sizes))
            nn2, best2, bad2 = ops.ahc_nearest_grouped(Sv, invd, group, max(sizes))
            assert torch.equal(nn, nn2) and torch.equal(_bits(best), _bits(best2)) and int(bad) == 0 == int(bad2)      # bitwise run to run
            nn, best = nn.cpu().numpy(), best.cpu().numpy()
            assert not np.isnan(best).any(), "the NaN of columns [d, ld) was read"
            want_nn, want_best = _alone(ops, Sv, invd, sizes)
            assert np.array_equal(nn, want_nn), f"d={d} ld={ld}: {int((nn != want_nn).sum())} neighbours differ"
            assert np.array_equal(best.view(np.int32), want_best.view(np.int32)), f"d={d} ld={ld}: scores differ in their bits"
            worst = 0.0
            for a, b in zip(bounds[:-1], bounds[1:]):
                local = np.where(nn[a:b] >= 0, nn[a:b] - a, -1)
                worst = max(worst, A.check_nearest(local, best[a:b], S[a:b, :d], inv[a:b], d))
            print(f"grouped nearest n={n} d={d} ld={ld}: error / bound {worst:.4f}")
            mutual = (nn >= 0) & (nn[np.maximum(nn, 0)] == np.arange(n))                      # reciprocal pairs carry the same bits
            assert mutual.any() and np.array_equal(best[mutual].view(np.int32), best[nn[mutual]].view(np.int32))
            alone = np.flatnonzero(np.asarray(sizes) == 1)
            assert np.all(nn[bounds[alone]] == -1) and np.all(best[bounds[alone]] == -np.inf)


def test_the_mask_keeps_every_pair_inside_its_group(dev):
    """Copies of one unit row: three in group 0, one in group 1 (the same tile), two in group 3 (tiles 3 and 4 away from the first).
    Their mutual score is the largest there is and the ungrouped kernel takes it across the groups; the grouped one never does: a copy
    pairs with the lowest copy of its own group, and the lone copy of group 1 with an ordinary row of group 1."""
    from speech_diarization_amd import ops
    sizes = [60, 60, 300, 100, 80]                                  # groups at rows 0, 60, 120, 420, 520; W = 3 of T - 1 = 4
    n, d = sum(sizes), 192
    X = A.unit_rows(np.random.default_rng(5).standard_normal((n, d)))
    copies = [3, 10, 40, 70, 430, 500]
    X[copies] = X[3]
    Xd, ones, group = torch.from_numpy(X).to(dev), torch.ones(n, device=dev), _group(dev, sizes)
    nn, best, bad = ops.ahc_nearest_grouped(Xd, ones, group, max(sizes))
    nn, best, g = nn.cpu().numpy(), best.cpu().numpy(), group.cpu().numpy()
    assert int(bad) == 0 and np.array_equal(g[nn], g)
    assert nn[3] == 10 and nn[10] == 3 and nn[40] == 3 and nn[430] == 500 and nn[500] == 430
    same = [3, 10, 40, 430, 500]
    assert len(set(best[same].view(np.int32).tolist())) == 1 and abs(float(best[3]) - 1.0) <= 1e-6
    assert 60 <= nn[70] < 120 and best[70] < 0.5                    # the largest score of row 70 lies outside its group and is not taken
    want_nn, want_best = _alone(ops, Xd, ones, sizes)
    assert np.array_equal(nn, want_nn) and np.array_equal(best.view(np.int32), want_best.view(np.int32))
    full_nn, full_best = ops.ahc_nearest(Xd, ones)                  # the test bites: without the mask row 70 and the far copies pair with row 3
    full_nn = full_nn.cpu().numpy()
    assert full_nn[70] == 3 and full_nn[430] == 3 and full_nn[500] == 3 and float(full_best[70]) == float(best[3])


# ------------------------------------------------------------------ the promise

def test_a_broken_promise_is_reported(dev):
    """`bad` is non-zero when a group has more rows than max_group or `group` decreases somewhere, and 0 at the exact bound; with one
    group over everything and max_group = n the entry is `ops.ahc_nearest`, bit for bit."""
    from speech_diarization_amd import ops
    sizes = [5, 300, 129, 40]
    n, d = sum(sizes), 190
    S, count, inv = A.grid_case(n, d, 192, seed=9)
    Sv, invd = _on(dev, S, d, inv)
    group = _group(dev, sizes)
    assert int(ops.ahc_nearest_grouped(Sv, invd, group, 300)[2]) == 0                      # the exact bound
    assert int(ops.ahc_nearest_grouped(Sv, invd, group, 301)[2]) == 0 and int(ops.ahc_nearest_grouped(Sv, invd, group, 10 ** 9)[2]) == 0
    assert int(ops.ahc_nearest_grouped(Sv, invd, group, 299)[2]) != 0                      # one below the largest group
    assert int(ops.ahc_nearest_grouped(Sv, invd, group, 1)[2]) != 0
    for at, value in ((150, 0), (n - 1, 2), (1, -4)):                                      # one descent: in the middle, at the end, at the start
        down = group.clone()
        down[at] = value
        assert AG.promise_broken(down.cpu().numpy(), 300) and int(ops.ahc_nearest_grouped(Sv, invd, down, 300)[2]) != 0, at
    assert int(ops.ahc_nearest_grouped(Sv, invd, group, 300)[2]) == 0                      # `bad` is set to 0 first, every call
    for m in (1, 129, 700):
        S, count, inv = A.grid_case(m, d, 192, seed=m)
        Sv, invd = _on(dev, S, d, inv)
        nn, best, bad = ops.ahc_nearest_grouped(Sv, invd, torch.zeros(m, dtype=torch.int32, device=dev), m)
        want_nn, want_best = ops.ahc_nearest(Sv, invd)
        assert int(bad) == 0 and torch.equal(nn, want_nn) and torch.equal(_bits(best), _bits(want_best)), m


# ------------------------------------------------------------------ exact buffer sizes, guard bands (style of tests/test_gpu_ahc.py)

EDGE_SHAPES = [(1, 4, 4, 1), (5, 7, 8, 2), (129, 190, 192, 129), (257, 192, 192, 3), (1000, 192, 196, 300)]      # (n, d, ld, max_group)


@pytest.mark.parametrize("n,d,ld,max_group", EDGE_SHAPES)
def test_entry_at_exact_buffer_sizes(dev, n, d, ld, max_group):
    """Every buffer ends at its last element (the last row of `sums` at column d), the workspace has exactly the bytes of the formula:
    one byte less is refused, nothing outside is written, the NaN of the padding columns [d, ld) is never read, and the results are
    those of the wrapper's own allocations."""
    from speech_diarization_amd import _native as N, ops
    lib = N.load()
    sizes = [max_group] * (n // max_group) + ([n % max_group] if n % max_group else [])
    S, count, inv = A.grid_case(n, d, ld, seed=n + d)
    Sv, invd = _on(dev, S, d, inv)
    group_h = AG.group_of(sizes)
    want_nn, want_best, want_bad = ops.ahc_nearest_grouped(Sv, invd, torch.from_numpy(group_h).to(dev), max_group)
    assert int(want_bad) == 0 and not bool(torch.isnan(want_best).any())
    flat = torch.from_numpy(S.reshape(-1)[: (n - 1) * ld + d].copy())
    need = int(lib.sd_ahc_nearest_grouped_workspace_bytes(n, d, max_group))
    assert need == AG.workspace_bytes(n, max_group)
    for poison in G.POISONS:
        gS = G.guarded_from(flat, dev, "sums")
        gi = G.guarded_from(torch.from_numpy(inv), dev, "inv_count")
        gg = G.guarded_from(torch.from_numpy(group_h), dev, "group")
        gn, gb, gbad = G.guarded(n * 4, poison, dev, "nn"), G.guarded(n * 4, poison, dev, "best"), G.guarded(4, poison, dev, "bad")
        gw = G.guarded(need, poison, dev, "ws")
        args = (gS.ptr, ld, n, d, gi.ptr, gg.ptr, max_group, gn.ptr, gb.ptr, gbad.ptr, gw.ptr)
        assert CAP.call("sd_ahc_nearest_grouped_f32", *args, need - 1) == -3                 # one byte short
        N.check(CAP.call("sd_ahc_nearest_grouped_f32", *args, need), "sd_ahc_nearest_grouped_f32")
        torch.cuda.synchronize()
        G.assert_guards_intact(gS, gi, gg, gn, gb, gbad, gw)
        assert torch.equal(gn.view(torch.int32), want_nn) and torch.equal(_bits(gb.view(torch.float32)), _bits(want_best)), poison
        assert int(gbad.view(torch.int32)[0]) == 0, poison


def test_lib_refuses_on_the_device_too(dev):
    """Refusals of tests/test_ahc_grouped_rules.py with real device buffers: nothing is written."""
    from speech_diarization_amd import _native as N
    lib = N.load()
    S, inv = torch.ones((64, 192), device=dev), torch.ones(64, device=dev)
    group = torch.zeros(64, dtype=torch.int32, device=dev)
    nn, best = torch.full((64,), 7, dtype=torch.int32, device=dev), torch.full((64,), 7.0, device=dev)
    bad = torch.full((1,), 7, dtype=torch.int32, device=dev)
    ws = torch.empty(int(lib.sd_ahc_nearest_grouped_workspace_bytes(64, 192, 64)), dtype=torch.uint8, device=dev)

    def call(sums=S.data_ptr(), ld=192, n=64, d=192, max_group=64, ws_bytes=ws.numel()):
        return lib.sd_ahc_nearest_grouped_f32(sums, ld, n, d, inv.data_ptr(), group.data_ptr(), max_group, nn.data_ptr(), best.data_ptr(),
                                              bad.data_ptr(), ws.data_ptr(), ws_bytes, None)
    assert call(ld=190, d=190) == -1 and call(sums=S.data_ptr() + 4, n=63) == -1 and call(max_group=0) == -1 and call(ws_bytes=ws.numel() - 1) == -3
    torch.cuda.synchronize()
    assert bool((nn == 7).all()) and bool((best == 7.0).all()) and int(bad) == 7
    assert call() == 0
    torch.cuda.synchronize()
    assert float(best[5]) == 192.0 and int(nn[0]) == 1 and int(nn[5]) == 0 and int(bad) == 0


# ------------------------------------------------------------------ the driver

@pytest.mark.parametrize("thr", AG.DRIVER_THRESHOLDS)
def test_driver_equals_every_recording_alone(dev, thr):
    """The recordings of tests/test_ahc_grouped_rules.py on the device: labels equal `ahc_cosine_rows` per recording exactly (the
    arithmetic is the same bits, so this needs no margin), the rounds are the maximum of the recordings' rounds."""
    from speech_diarization_amd import ahc_gpu
    recs = AG.driver_recordings(thr)
    sizes = [len(x) for _, x in recs]
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    Xd = torch.from_numpy(np.concatenate([x for _, x in recs])).to(dev)
    labels, info = ahc_gpu.ahc_cosine_groups(Xd, sizes, thr, return_info=True)
    rounds = []
    for (f, x), a, b, got, clusters in zip(recs, bounds[:-1], bounds[1:], labels, info["clusters"]):
        want, inf = ahc_gpu.ahc_cosine_rows(Xd[a:b], thr, return_info=True)
        assert np.array_equal(got, want), (f, len(x), int((got != want).sum()))
        assert clusters == inf["clusters"]
        rounds.append(inf["rounds"])
    print(f"thr={thr}: rounds alone {rounds}, together {info['rounds']}; clusters {info['clusters']}; gram_tiles {info['gram_tiles']}")
    assert info["rounds"] == max(rounds)
    assert [got.tolist() for (f, _), got in zip(recs, labels) if f is None] == [[0, 0], [], [0]]
    again = ahc_gpu.ahc_cosine_groups(Xd, sizes, thr)
    assert all(np.array_equal(p, q) for p, q in zip(labels, again))


def test_driver_refuses_a_nan_row_before_a_launch(dev):
    from speech_diarization_amd import ahc_gpu
    X = torch.from_numpy(A.family_rows(400)[0]).to(dev)
    X[17, 3] = float("nan")
    with launches() as log:
        with pytest.raises(ValueError, match="finite"):
            ahc_gpu.ahc_cosine_groups(X, [100, 300], 0.3)
    assert log == {}


# ------------------------------------------------------------------ scale

def _same_partition(got, want):
    from speech_diarization_amd import cluster
    return np.array_equal(cluster.relabel_by_first_appearance(got), cluster.relabel_by_first_appearance(want))


def test_scale_a_folder_of_65_recordings(dev):
    """64 recordings of 300 planted rows (3 speakers each, different seeds) and one of 3 001: every recording recovers its planted
    partition, and the first pass computes fewer than twice the tiles of the recordings' own triangles (the band skips what no
    recording reaches; a full walk over the 22 201 rows would be 15 225 tiles)."""
    from speech_diarization_amd import ahc_gpu
    parts = [R.planted_rows(300, 3, 0.5, 100 + s, dtype=np.float32) for s in range(64)]
    parts.insert(10, R.planted_rows(3001, 3, 0.5, 99, dtype=np.float32))
    sizes = [len(x) for x, _ in parts]
    Xd = torch.from_numpy(np.concatenate([x for x, _ in parts])).to(dev)
    labels, info = ahc_gpu.ahc_cosine_groups(Xd, sizes, 0.3, return_info=True)
    print(f"{len(sizes)} recordings, {sum(sizes)} rows: {info['rounds']} rounds, gram_tiles {info['gram_tiles']}")
    assert info["clusters"] == [3] * 65
    for i, ((_, planted), got) in enumerate(zip(parts, labels)):
        assert _same_partition(got, planted), i
    _, first = ahc_gpu.ahc_cosine_groups(Xd, sizes, 1.5, return_info=True)                  # above every score: the first pass alone
    triangles = sum(t * (t + 1) // 2 for t in (-(-m // 128) for m in sizes))
    print(f"first pass: {first['gram_tiles']} tiles, the recordings' triangles {triangles}")
    assert first["rounds"] == 0 and 0 < first["gram_tiles"] < 2 * triangles


# ------------------------------------------------------------------ the pipeline

def _small_sd(width=128):
    from speech_diarization_amd import synth
    return synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(width))


@pytest.fixture()
def small_encoder(dev):
    """The small seeded encoder of tests/test_gpu_ahc.py."""
    from speech_diarization_amd import ecapa_annote, speech_encode
    enc = speech_encode.HipEcapaEncoder(_small_sd(), dev)
    speech_encode.using_ecapa_encoder.cache_clear()
    orig = speech_encode.using_ecapa_encoder
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = lambda device="cuda": enc
    yield enc
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = orig


EMBEDDING_BAR = 1e-9       # tests/test_gpu_configs.py::test_reference_batch_sizes_agree_with_a_small_batch_and_the_oracle, f32: one batch size against another


def test_rttms_are_byte_identical_to_one_recording_at_a_time(small_encoder, tmp_path):
    """A: 60 s, 2 voices, seed 0 (tests/test_gpu_ahc.py records its cut margin as 0.234 at 0.70).  B: 40 s, 3 voices, seed 1: its cut
    margin at 0.70 is 0.201 on the float64 oracle's embeddings of the same windows (seeds 1 .. 5 give 0.201, 0.141, 0.206, 0.157, 0.212,
    3 speakers each).  C: 5 s of silence.  D: 1.2 s, shorter than one window.  The embeddings of a shared launch differ from a lone
    launch by f32 rounding (other kernels at other batch sizes), so the inputs are conditioned first: every recording's host affinity
    has no merge height within CUT_MARGIN of the cut, and the two routes' embeddings agree row by row to the bar one batch size is
    held to against another."""
    from speech_diarization_amd import audio_io, cluster, diarization_baseline as db, ops, synth
    thr = 0.70
    conv_a, conv_b = synth.synthetic_conversation(60.0, 2, seed=0), synth.synthetic_conversation(40.0, 3, seed=1)
    speech_a = db._speech_regions(conv_a.wav.astype(np.float32), conv_a.sr, 0.35, 0.1)
    a0 = int(round(speech_a[0][0] * conv_a.sr))
    waves = {"a": conv_a.wav, "b": conv_b.wav, "c": np.zeros(5 * 16000, np.float32), "d": conv_a.wav[a0:a0 + int(1.2 * 16000)]}
    wavs = []
    for name, w in waves.items():
        wavs.append(tmp_path / f"{name}.wav")
        audio_io.write_wav16(wavs[-1], w, 16000)
    alone = [db.diarize_audio(w, 0.35, 0.1, 2, 6, rttm_filepath=w.with_suffix(".alone.rttm"), clustering="ahc_gpu", clustering_threshold=thr,
                              return_details=True) for w in wavs]
    windows = [len(det["labels"]) for _, det in alone]
    assert windows[0] == 119 and windows[1] >= 60 and windows[2] == 0 and windows[3] == 1, windows
    for name, (_, det) in zip(waves, alone):
        if len(det["labels"]) >= 2:
            K = ops.cosine_affinity(torch.from_numpy(cluster.center(det["embeddings"])).cuda()).cpu().numpy()
            margin = A.cut_margin(K, thr)
            print(f"recording {name}: {len(det['labels'])} windows, {len(set(det['labels'].tolist()))} speakers, cut margin {margin:.3f}")
            assert margin > A.CUT_MARGIN, (name, margin)
    assert [len(set(det["labels"].tolist())) for _, det in alone] == [2, 3, 0, 1]
    many = db.diarize_audios(wavs, 0.35, 0.1, 2, 6, rttm_filepaths=[w.with_suffix(".many.rttm") for w in wavs], clustering_threshold=thr,
                             return_details=True)
    assert len(many) == 4
    for name, w, (seg_1, det_1), (seg_m, det_m) in zip(waves, wavs, alone, many):
        e1, em = det_1["embeddings"].astype(np.float64), det_m["embeddings"].astype(np.float64)
        assert e1.shape == em.shape
        if len(e1):
            dist = 1.0 - (e1 * em).sum(1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(em, axis=1))
            print(f"recording {name}: shared launch against lone launch, largest row-wise cosine distance {dist.max():.2e}")
            assert dist.max() < EMBEDDING_BAR, (name, dist.max())
        assert w.with_suffix(".many.rttm").read_bytes() == w.with_suffix(".alone.rttm").read_bytes(), name
        assert seg_m == seg_1 and np.array_equal(det_m["labels"], det_1["labels"]), name
        assert det_m["speech"] == det_1["speech"] and det_m.get("affinity") is None
    assert many[2][0] == [] and wavs[2].with_suffix(".many.rttm").read_bytes() == b""
    hp = db.DiarizationParameters(min_speakers=2, max_speakers=6, clustering_threshold=thr)
    diarizer = db.Diarizer(hp, clustering="ahc_gpu")
    assert diarizer.diarize_many(wavs) == [diarizer.diarize(w, None) for w in wavs]
