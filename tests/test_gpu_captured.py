"""Every launching entry of libsd_hip.so, captured in a hipGraph and replayed twice, does what it does as an eager call.

Every header under include/ promises for every entry that takes an `sd_stream_t` that the call is asynchronous on `stream`, never
allocates and never synchronises.  The rest of the GPU suite launches on the default stream, where a kernel or memset issued on
stream 0 instead of `stream`, a synchronising or allocating call in a launch path, device state one call leaves behind for the next
(a counter, a `bad` flag, a max key) and anything that behaves differently as a graph node are all invisible.

CAPTURED maps an entry to its cases; a case is (id, fn(dev)) and `fn` is an EXISTING guarded helper or test body at one of its own
smallest shapes that still cross a tile boundary: a case of tests/test_gpu_buffer_edges.py's CASES, or the exact-buffer-size test of
the entry's own module.  Per case (tests/helpers/captured.py has the protocol):
  * eager: `fn` on the default stream, with all its own assertions (guards, neighbours, references at the operator's bar, launch log);
  * replayed: `fn` again inside `replaying(entry)`: every launch of the entry is captured with torch.cuda.graph, the guarded buffers
    are put back to their state before the call, the graph is replayed, the buffers put back again, the graph replayed again (bit for
    bit the first replay), and `fn`'s own assertions then hold on what the second replay wrote; as many launches were captured as ran
    eagerly, and as many were refused;
  * equal: after every launch, every guarded buffer of the case that is no workspace holds the bytes it held in the eager run.
tests/test_captured_rules.py (no GPU) reads the entry names from the headers and fails for one that is not a key of CAPTURED.

The product drivers that keep `ops.Workspace` objects and read counts back between launches run once more on a side stream."""
import os
import sys
import time

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
sys.path.insert(0, HERE)
import captured as CAP  # noqa: E402
import guarded as G  # noqa: E402

import test_gpu_ahc as AHC  # noqa: E402
import test_gpu_ahc_cut as CUT  # noqa: E402
import test_gpu_ahc_grouped as AHG  # noqa: E402
import test_gpu_buffer_edges as B  # noqa: E402
import test_gpu_diag as DG  # noqa: E402
import test_gpu_hdbscan as HD  # noqa: E402
import test_gpu_hdbscan_grouped as HDG  # noqa: E402
import test_gpu_hdbscan_labels as HL  # noqa: E402
import test_gpu_kmeans as KM  # noqa: E402
import test_gpu_scd as SCD  # noqa: E402
import test_gpu_spectral as SP  # noqa: E402
import test_gpu_turns as TU  # noqa: E402
import test_gpu_vad as VD  # noqa: E402
from kernel_selection import CONV_KERNELS  # noqa: E402

pytestmark = pytest.mark.gpu

CAPTURED = {}


def _edges(entry, *cids):
    """Cases of tests/test_gpu_buffer_edges.py, by id."""
    table = dict(B.CASES[entry])
    CAPTURED.setdefault(entry, []).extend((cid, table[cid]) for cid in cids)


def _from(entry, cid, fn, *args):
    """A test body of the entry's own module at one of its own parameters: fn(dev, *args); `_nodev`: fn(*args)."""
    CAPTURED.setdefault(entry, []).append((cid, lambda dev: fn(dev, *args)))


def _nodev(entry, cid, fn, *args):
    CAPTURED.setdefault(entry, []).append((cid, lambda dev: fn(*args)))


# ====================================================================== include/sd_hip.h: cases out of CASES

_edges("sd_fbank_f32", "speechbrain-one-row-n640", "torchaudio-n801", "generic-sr8000")
_edges("sd_fbank_windows_f32", "generic-8k", "torchaudio-one-launch")
_edges("sd_fbank_lens_f32", "floor-n640")
_edges("sd_fbank_packed_f32", "one-launch-only")
_edges("sd_wav_lens_frames", "counts")
_edges("sd_conv1d_cl_f32", *[f"plain-{sel}-0" for sel in CONV_KERNELS])
_edges("sd_conv1d_cl_f16", "plain-auto-0", "plain-wide256-0")
_edges("sd_conv1d_cl_split16", "narrow-0", "wide-out-split")
_edges("sd_conv1d_cl_packed_f32", "one-span", "stem-129-rows")
_edges("sd_split16_pack_f32", "c36")
_edges("sd_seg_gemm_f32", "M7-K1000-N36", "M5-K256-N64", "M32-K6144-N128")
_edges("sd_colstat_finish_dt", "f32-auto", "f16")
_edges("sd_res2net_chain_f16", "B5-T5-n3-ld520")
for _e in ("sd_seg_mean_f32", "sd_seg_mean_std_f32", "sd_se_scale_residual_f32", "sd_asp_pool_f32"):
    _edges(_e, "B3-T50-C100")
for _e in ("sd_seg_mean_std_dt", "sd_seg_mean_std_lens_dt", "sd_seg_mean_std_packed_dt", "sd_se_scale_residual_dt", "sd_se_scale_residual_packed_dt",
           "sd_asp_pool_dt", "sd_asp_pool_lens_dt", "sd_asp_pool_packed_dt"):
    _edges(_e, "f32-B3-T50-C100", "f16-B3-T50-C100")
for _e in ("sd_asp_attend_pool_dt", "sd_asp_attend_pool_lens_dt"):
    _edges(_e, "f32-T7", "f16-T7", "split16-T7")
_edges("sd_ecapa_forward_f32", "small64-f32-B31-T5", "small64-f32s-B31-T5", "small64-f32ns-B31-T5", "default-f32-B37-T7")
_edges("sd_ecapa_forward_f16", "small64-f16-B31-T5")
_edges("sd_ecapa_forward_lens_f32", "small128-f32-B31-T5")
_edges("sd_ecapa_forward_lens_f16", "small128-f16-B31-T5")
_edges("sd_ecapa_forward_packed_f32", "small64-B31-mixed")
_edges("sd_l2norm_rows_f32", "n1-d7", "n129-d50-padded")
_edges("sd_cosine_affinity_f32", "n1-d7", "n129-d50")
_edges("sd_cosine_affinity_rows_f32", "n129-d50-last-rows")
_edges("sd_cosine_affinity_rows_split16", "n129-d50-last-rows")
for _e in ("sd_adjacent_cosine_f32", "sd_sim_argmax_f32"):
    _edges(_e, "n2-d7-k1", "n129-d50-k3-strided")
_edges("sd_topk_mean_std_f32", "rows2-n50-k200", "rows4-n257-k1")
_edges("sd_asnorm_combine_f32", "nq37-nr129")
_edges("sd_viterbi_f32", "T1-K3", "T129-K8")


# ====================================================================== the other ten headers: the modules' own guarded bodies

# sd_hip_ahc.h.  The merge of (129, 190, 192) at the median score of the reciprocal pairs merges several pairs, so `n_merged` is
# non-zero after every replay; the case below it sets `bad` of the grouped entry.
for _n, _d, _ld in ((5, 7, 8), (129, 190, 192)):
    for _e in ("sd_ahc_nearest_f32", "sd_ahc_merge_f32"):
        _from(_e, f"n{_n}-d{_d}-ld{_ld}", AHC.test_both_entries_at_exact_buffer_sizes, _n, _d, _ld)
for _n, _d, _ld, _mg in ((5, 7, 8, 2), (129, 190, 192, 129), (257, 192, 192, 3)):
    _from("sd_ahc_nearest_grouped_f32", f"n{_n}-d{_d}-ld{_ld}-g{_mg}", AHG.test_entry_at_exact_buffer_sizes, _n, _d, _ld, _mg)


def _ahc_grouped_sets_bad(dev):
    """One group of 129 rows under max_group = 64 and a `group` that decreases, on guarded buffers of the documented sizes: `bad` is
    non-zero after the call whatever it held before, and every guard band is intact."""
    import ahc_ref as A
    from speech_diarization_amd import _native as N
    n, d, ld = 129, 190, 192
    S, _, inv = A.grid_case(n, d, ld, seed=3)
    flat = torch.from_numpy(S.reshape(-1)[: (n - 1) * ld + d].copy())
    down = np.zeros(n, np.int32)
    down[:40] = 1
    for group, max_group in ((np.zeros(n, np.int32), 64), (down, 129)):
        need = int(N.load().sd_ahc_nearest_grouped_workspace_bytes(n, d, max_group))
        for poison in G.POISONS:
            gS, gi = G.guarded_from(flat, dev, "sums"), G.guarded_from(torch.from_numpy(inv), dev, "inv_count")
            gg = G.guarded_from(torch.from_numpy(group), dev, "group")
            gn, gb, gbad = G.guarded(n * 4, poison, dev, "nn"), G.guarded(n * 4, poison, dev, "best"), G.guarded(4, poison, dev, "bad")
            gw = G.guarded(need, poison, dev, "ws")
            N.check(CAP.call("sd_ahc_nearest_grouped_f32", gS, ld, n, d, gi, gg, max_group, gn, gb, gbad, gw, need), "sd_ahc_nearest_grouped_f32")
            torch.cuda.synchronize()
            G.assert_guards_intact(gS, gi, gg, gn, gb, gbad, gw)
            flag = int(gbad.view(torch.int32)[0])
            assert flag != 0 and flag != int(np.frombuffer(bytes([poison] * 4), np.int32)[0]), (max_group, poison, flag)


CAPTURED["sd_ahc_nearest_grouped_f32"].append(("n129-bad-set", _ahc_grouped_sets_bad))

# sd_hip_cut.h
_nodev("sd_ahc_cut_grouped", "two", CUT.test_entry_at_exact_buffer_sizes, (5, 64))
_nodev("sd_ahc_cut_grouped", "four", CUT.test_entry_at_exact_buffer_sizes, (257, 0, 1000, 1))

# sd_hip_diag.h
for _e in ("sd_whiten_stats_f64", "sd_whiten_apply_f64", "sd_label_centroids_f32"):
    _from(_e, "n130-d20-ld24", DG.test_no_entry_leaves_its_buffers, 130, 20, 24)
    _from(_e, "n514-d190-ld192", DG.test_no_entry_leaves_its_buffers, 514, 190, 192)

# sd_hip_hdbscan.h.  The grouped body runs its two broken promises (a decreasing `group`, a group above max_group) on the same guarded
# buffers, so `bad` of both grouped entries is non-zero after those replays.
for _n, _d, _ld in ((3, 7, 8), (129, 190, 192)):
    for _e in ("sd_hdb_core_f32", "sd_hdb_outgoing_f32"):
        _from(_e, f"n{_n}-d{_d}-ld{_ld}", HD.test_both_entries_at_exact_buffer_sizes, _n, _d, _ld)
for _shape in ((129, 190, 192, 129, 16), (257, 192, 192, 3, 2)):
    for _e in ("sd_hdb_core_grouped_f32", "sd_hdb_outgoing_grouped_f32"):
        _from(_e, "n%d-d%d-ld%d-g%d-k%d" % _shape, HDG.test_entries_at_exact_buffer_sizes, *_shape)


# sd_hip_kmeans.h
def _kmeans(dev):
    """Recordings of 63, 64, 65 and 255 rows in one launch, twice, against scikit-learn (the inputs of test_every_flag)."""
    good = KM.KR.gpu_cases(2)[1:5]
    want = KM._reference("flags", good)
    KM._check(KM._twice(dev, [c[0] for c in good], [c[1] for c in good], KM._draws(good)), good, want)


CAPTURED["sd_kmeans_grouped_f64"] = [("n63-64-65-255-d2", _kmeans)]

# sd_hip_scd.h
_from("sd_scd_split_grouped_f32", "dim5-ld8", SCD.test_short_segments_and_the_smallest_peak, 5, 3)
_from("sd_scd_split_grouped_f32", "dim192", SCD.test_short_segments_and_the_smallest_peak, 192, 0)

# sd_hip_spectral.h
for _n, _ld in ((5, 8), (129, 131), (129, 132)):
    _from("sd_affinity_degree_f32", f"n{_n}-ld{_ld}", SP.test_degree_at_exact_buffer_sizes, _n, _ld)
for _n, _ld in ((129, 131), (129, 132)):                                # scalar and 16-byte loads of K; 24 launches each
    _from("sd_affinity_apply_f32", f"n{_n}-ld{_ld}", SP.test_apply_at_exact_buffer_sizes, _n, _ld)

# sd_hip_tree.h
_TREES = {}


def _tree_labels(dev, kind):
    if not _TREES:
        _TREES.update({name: (lo, hi, dist) for name, lo, hi, dist in HL.T.random_cases()})
    HL.test_a_broken_recording_is_reported_and_the_others_are_not_touched(_TREES, kind)


_from("sd_tree_labels_grouped", "cycle", _tree_labels, "cycle")
_from("sd_tree_labels_grouped", "nan", _tree_labels, "nan")

# sd_hip_turns.h
_from("sd_turns_grouped", "smallest", TU.test_one_window_one_frame_and_a_window_without_a_frame)
_from("sd_turns_grouped", "pass-boundary", TU.test_regions_across_the_pass_boundary)
_from("sd_turns_grouped", "workspace-tables", TU.test_recordings_around_the_size_of_the_lds_tables, TU.T.LDS_WINDOWS + 1, TU.WS)

# sd_hip_vad.h
_from("sd_vad_energy_grouped_f32", "win30-hop7", VD.test_energy_against_the_float64_statement, 30, 7)
_from("sd_vad_energy_grouped_f32", "win480-hop160", VD.test_energy_against_the_float64_statement, 480, 160)
_from("sd_vad_segments_grouped", "thresholds-no-mask", VD.test_other_thresholds_and_no_mask)


# ====================================================================== the table, run

_TIMES = {}


@pytest.mark.parametrize("entry,cid", [(e, cid) for e in CAPTURED for cid, _ in CAPTURED[e]])
def test_captured(dev, entry, cid):
    fn = dict(CAPTURED[entry])[cid]
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        with CAP.observing(entry) as eager:
            fn(dev)
        assert eager.launches > 0, f"{entry}[{cid}] never launches {entry}"
        with CAP.replaying(entry) as replayed:
            fn(dev)
        assert (replayed.launches, replayed.refused) == (eager.launches, eager.refused), \
            f"{entry}[{cid}]: {eager.launches} launches and {eager.refused} refusals eagerly, {replayed.launches} and {replayed.refused} captured"
        CAP.same_records(eager.records, replayed.records, entry)
    _TIMES[(entry, cid)] = time.perf_counter() - t0


def test_print_how_many_entries_and_cases_ran(capsys):
    """Runs after the table: one line, past pytest's capture, with the entries and cases that ran in this session and the slowest case."""
    assert set(_TIMES) <= {(e, cid) for e in CAPTURED for cid, _ in CAPTURED[e]}
    line = "captured: no case of the table ran in this session"
    if _TIMES:
        slow = max(_TIMES, key=_TIMES.get)
        line = (f"captured: {len({e for e, _ in _TIMES})} entries, {len(_TIMES)} cases; slowest {slow[0]}[{slow[1]}] "
                f"{_TIMES[slow]:.2f} s (eager + capture + two replays per launch)")
    with capsys.disabled():
        print("\n" + line)


# ====================================================================== the drivers on a side stream

def _on_side_stream(fn):
    """fn() with a fresh stream current: the stream first waits for the current one, and the current one then waits for it."""
    here = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(here)
    with torch.cuda.stream(side):
        out = fn()
    here.wait_stream(side)
    torch.cuda.synchronize()
    return out


def _same_arrays(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) and np.asarray(x).dtype == np.asarray(y).dtype for x, y in zip(a, b))


def test_ahc_cosine_groups_on_a_side_stream(dev):
    from speech_diarization_amd import ahc_gpu
    import ahc_grouped_ref as AG
    thr = AG.DRIVER_THRESHOLDS[0]
    recs = AG.driver_recordings(thr)
    sizes = [len(x) for _, x in recs]
    Xd = torch.from_numpy(np.concatenate([x for _, x in recs])).to(dev)
    want = ahc_gpu.ahc_cosine_groups(Xd, sizes, thr)
    assert _same_arrays(_on_side_stream(lambda: ahc_gpu.ahc_cosine_groups(Xd, sizes, thr)), want)


def test_hdbscan_rows_groups_with_labels_on_a_side_stream(dev):
    from speech_diarization_amd import hdbscan_gpu
    parts = [HDG.H.planted(300, 3, 0.5, 100 + s, 0) for s in range(3)] + [HDG.H.planted(129, 3, 0.5, 5, 4)]
    sizes = [len(x) for x in parts]
    Xd = torch.from_numpy(np.concatenate(parts)).to(dev)
    for setting in ((2, None, True), (6, 3, False)):
        want = hdbscan_gpu.hdbscan_rows_groups(Xd, sizes, *setting)
        assert _same_arrays(_on_side_stream(lambda: hdbscan_gpu.hdbscan_rows_groups(Xd, sizes, *setting)), want), setting


def test_k_means_groups_on_a_side_stream(dev):
    from speech_diarization_amd import kmeans_gpu
    cases = KM.KR.gpu_cases(2)[1:4]
    X = np.concatenate([c[0] for c in cases])
    sizes, ks = [len(c[0]) for c in cases], [c[1] for c in cases]

    def run():
        return kmeans_gpu.k_means_groups(X, sizes, ks, [np.random.RandomState(c[2]) for c in cases])
    want = run()
    assert _same_arrays(_on_side_stream(run), want)
    for got, ref in zip(want, KM._reference("side", cases)):
        assert np.array_equal(got, ref[0])


def test_vad_segments_groups_on_a_side_stream(dev):
    from speech_diarization_amd import vad_gpu
    ys = VD._signals()
    want = vad_gpu.vad_segments_groups(ys)
    assert _on_side_stream(lambda: vad_gpu.vad_segments_groups(ys)) == want and sum(len(w) for w in want) > 20


def test_scd_split_rows_groups_on_a_side_stream(dev):
    from speech_diarization_amd import scd_gpu
    rs = np.random.RandomState(192)
    S = SCD.S
    rows = [S.rows_with_cosines([0.3], 192, rs), S.rows_with_cosines([0.9, 0.2, 0.9], 192, rs), S.rows_with_cosines([0.9, 0.3, 0.95, 0.5], 192, rs),
            S.rows_with_cosines(list(S.cosine_family("drops", 129, rs)), 192, rs)]
    first_row = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    starts = SCD._times(len(rows))
    ends = starts + np.array([1.2, 1.6, 1.8, 27.0])
    rows_dev = torch.from_numpy(np.concatenate(rows)).to(dev)
    want = scd_gpu.split_rows_groups(rows_dev, first_row, starts, ends, 200.0, 1.0, 100.0)
    assert _on_side_stream(lambda: scd_gpu.split_rows_groups(rows_dev, first_row, starts, ends, 200.0, 1.0, 100.0)) == want
    assert sum(k for k, _ in want) >= 2


def test_labels_to_turns_groups_on_a_side_stream(dev):
    from speech_diarization_amd import turns_gpu
    folder = [([(0.0, 2.0), (3.0, 4.0), (5.0, 8.0)], np.array([0.5, 1.0, 1.5, 6.0, 6.5, 7.0]), np.array([0, 0, 0, 2, 2, 2]), np.array([2, 2, 0, 0, -1, 2])),
              ([], None, None, np.zeros(0, int)),
              ([(0.5, 1.5), (2.0, 2.4)], np.zeros(0), np.zeros(0, np.int64), np.zeros(0, int)),
              ([(0.0, 80.0)], 0.125 + 0.25 * np.arange(300), np.zeros(300, np.int64), np.arange(300) // 7 % 3)]
    args = [list(x) for x in zip(*folder)]
    want = turns_gpu.labels_to_turns_groups(*args)
    got = _on_side_stream(lambda: turns_gpu.labels_to_turns_groups(*args))
    assert len(got) == len(want) == 4 and len(want[0][1]) == 5 and len(want[3][1]) > 40
    for (gl, gt), (wl, wt) in zip(got, want):
        assert np.array_equal(gl, wl) and gt == wt


def test_diar_diag_on_a_side_stream(dev):
    """`resegment` on the device (whitening statistics, centres, scores and the Viterbi path) on a side stream: labels, path and
    segments those of the default stream exactly, scores and centres at the bars of test_gpu_diag.py."""
    from speech_diarization_amd import diar_diag as dd
    import diag_cases as DC
    X, _ = DC.planted_lowrank(*DC.RESEGMENT_CASES[0])
    segs = [[i * 1.0, i * 1.0 + 0.8] for i in range(len(X))]
    Xd = torch.from_numpy(X).to(dev)
    for method in ("agglo", "hdbscan"):
        want = dd.resegment(Xd, segs, cluster=method, whiten=1, device=dev)
        got = _on_side_stream(lambda: dd.resegment(Xd, segs, cluster=method, whiten=1, device=dev))
        assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["final_labels"], want["final_labels"])
        assert got["segments"] == want["segments"]
        ws, gs = want["scores"].cpu().numpy().astype(np.float64), got["scores"].cpu().numpy().astype(np.float64)
        assert np.abs(ws - gs).max() <= 1e-4 * np.abs(ws).max()
        assert np.abs(np.asarray(got["centers"]) - np.asarray(want["centers"])).max() <= 1e-5
