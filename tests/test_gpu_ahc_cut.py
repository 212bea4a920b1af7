"""The bounded cut of the AHC route on the GPU (include/sd_hip_cut.h, sd_ahc_cut_grouped): exact integer equality of labels, cluster
counts and verdicts with the numpy statement of tests/helpers/ahc_cut_ref.py on synthetic merge logs, guard bands at exact buffer
sizes, every cause of `bad`, the bounded drivers of `ahc_gpu` against the scipy oracle, and `diarize_audios(..., speaker_bounds=True)`
against `diarize_audio` per recording.  Every run is held to its kernel by the launch log."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import ahc_cut_ref as CR  # noqa: E402
import ahc_grouped_ref as AG  # noqa: E402
import guarded as G  # noqa: E402
import launch_log as L  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import ahc_gpu, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNEL = "ahc_cut_grouped_kernel"

_LOGS = {}


def _log(n, seed=0, full=True, equal_keys=False):
    """The synthetic log of a recording, made once per session."""
    at = (n, seed, full, equal_keys)
    if at not in _LOGS:
        _LOGS[at] = CR.random_log(n, seed, full, equal_keys)
    return _LOGS[at]


def _run(packed, thr, lo_b, hi_b):
    """One launch over the packed logs, twice: identical bits run to run -> (labels, clusters, bad) as numpy."""
    up = [torch.from_numpy(a).to(DEV) for a in packed]
    bounds = [torch.from_numpy(np.asarray(b, np.int32)).to(DEV) for b in (lo_b, hi_b)]
    runs = []
    for _ in range(2):
        with L.expect_launches(exactly={KERNEL}) as log:
            out = ops.ahc_cut_grouped(*up, thr, *bounds)
            runs.append([t.cpu().numpy() for t in out])
        assert log == {KERNEL: 1}, log
    for first, second in zip(*runs):
        assert first.dtype == np.int32 and first.tobytes() == second.tobytes()
    return runs[0]


def _check(logs, sizes, thr, lo_b, hi_b):
    """A launch against the numpy statement, exactly -> (labels, clusters, bad)."""
    packed = CR.pack(logs, sizes)
    got = _run(packed, thr, lo_b, hi_b)
    want = CR.cut_numpy(*packed, thr, lo_b, hi_b)
    for name, g, w in zip(("labels", "clusters", "bad"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), (name, int((g != w).sum()))
    return got


# ------------------------------------------------------------------ 1. the entry against the numpy statement

ORDERS = {"issue": CR.SIZES, "other": (1000, 1, 257, 0, 64, 2, 255, 1, 65, 3, 256, 63, 5)}


@pytest.mark.parametrize("equal_keys", [False, True], ids=["distinct", "ties"])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_recordings_of_every_size_in_one_launch(order, equal_keys):
    """0, 1 and 2 rows, both sides of 64 and of 256 (a wave, the workgroup), 1000: bounds that bind at the minimum, at the maximum,
    min = max, and bounds that do not bind, with cos_thr exactly a key of the log (the comparison is strict).  With `ties` the keys
    come from four values, so parents and children carry equal keys and the position decides."""
    sizes = ORDERS[order]
    assert sorted(sizes) == sorted(CR.SIZES)
    logs = [_log(n, i, equal_keys=equal_keys) for i, n in enumerate(sizes)]
    big = logs[sizes.index(1000)][2]
    thr = float(np.sort(big)[len(big) // 2])
    assert (big == np.float32(thr)).any() and 0 < (big > np.float32(thr)).sum() < len(big)
    seen = set()
    for name, (lo_b, hi_b) in CR.bounds_cases(sizes, logs, thr).items():
        labels, clusters, bad = _check(logs, sizes, thr, lo_b, hi_b)
        assert not bad.any(), (name, bad)
        at = sizes.index(1000)
        unbounded = 1000 - int((big > np.float32(thr)).sum())
        seen.add((name, int(np.sign(int(clusters[at]) - unbounded))))
        assert clusters[sizes.index(0)] == 0 and (clusters[[i for i, n in enumerate(sizes) if n == 1]] == 1).all()
    assert seen == {("min", 1), ("max", -1), ("equal", -1), ("free", 0)}          # each case is what its name says


def test_a_recording_past_any_lds_size():
    """5 000 rows between small neighbours: nothing in the kernel is sized by the recording."""
    sizes = (65, 5000, 3)
    logs = [_log(n, 7) for n in sizes]
    thr = float(np.sort(logs[1][2])[1700])
    for name, (lo_b, hi_b) in CR.bounds_cases(sizes, logs, thr).items():
        labels, clusters, bad = _check(logs, sizes, thr, lo_b, hi_b)
        assert not bad.any(), name
    assert _check(logs, sizes, float("-inf"), [1] * 3, [5000] * 3)[1].tolist() == [1, 1, 1]
    assert _check(logs, sizes, float("inf"), [1] * 3, [5000] * 3)[1].tolist() == [65, 5000, 3]


def test_short_and_empty_logs():
    """A log that stops early is legal while the bounds do not ask for more merges than it has; an empty log for a recording of several
    rows leaves every row a cluster."""
    sizes = (64, 257, 5, 2, 1000)
    logs = [_log(64, 3, full=False), _log(257, 3, full=False), (np.zeros(0, np.int32),) * 2 + (np.zeros(0, np.float32),), _log(2, 3), _log(1000, 3, full=False)]
    assert [len(l[2]) for l in logs] == [31, 128, 0, 1, 499]
    labels, clusters, bad = _check(logs, sizes, -2.0, [1] * 5, [64, 257, 5, 2, 1000])
    assert not bad.any() and clusters.tolist() == [33, 129, 5, 1, 501]
    labels, clusters, bad = _check(logs, sizes, 2.0, [1] * 5, [40, 129, 5, 1, 400])          # the last one's log is too short for its maximum
    assert bad.tolist() == [0, 0, 0, 0, 1] and clusters.tolist() == [40, 129, 5, 1, 0]
    labels, clusters, bad = _check(logs, sizes, 2.0, [1] * 5, [40, 129, 4, 1, 501])          # so is the empty one's
    assert bad.tolist() == [0, 0, 1, 0, 0] and (labels[64 + 257:64 + 257 + 5] == -1).all()


# ------------------------------------------------------------------ 2. guard bands

@pytest.mark.parametrize("sizes", [(257, 0, 1000, 1), (5, 64)], ids=["four", "two"])
def test_entry_at_exact_buffer_sizes(sizes):
    """Every buffer between guard bands, the outputs and the workspace at exactly their sizes and pre-filled with poison."""
    logs = [_log(n, 11) for n in sizes]
    packed = CR.pack(logs, sizes)
    rows, groups, merges = int(sum(sizes)), len(sizes), len(packed[2])
    thr = 0.25
    lo_b, hi_b = (np.asarray(b, np.int32) for b in CR.bounds_cases(sizes, logs, thr)["max"])
    need = int(N.load().sd_ahc_cut_workspace_bytes(rows, groups))
    assert need == 4 * rows
    names = ("lo", "hi", "key", "first_merge", "first_row", "min_clusters", "max_clusters")
    bufs = {k: G.guarded_from(torch.from_numpy(v), DEV, name=k) for k, v in zip(names, packed + (lo_b, hi_b))}
    labels, clusters, bad = (G.guarded(4 * n, 0x7B, DEV, name=k) for k, n in (("labels", rows), ("clusters", groups), ("bad", groups)))
    ws = G.guarded(need, 0xFF, DEV, name="ws")
    with L.expect_launches(exactly={KERNEL}):
        ops.launch("sd_ahc_cut_grouped", labels.raw, bufs["lo"].ptr, bufs["hi"].ptr, bufs["key"].ptr, bufs["first_merge"].ptr, bufs["first_row"].ptr,
                   groups, merges, rows, N.C.c_float(thr), bufs["min_clusters"].ptr, bufs["max_clusters"].ptr, labels.ptr, clusters.ptr, bad.ptr,
                   ws.ptr, need)
        torch.cuda.synchronize()
    G.assert_guards_intact(labels, clusters, bad, ws, *bufs.values())
    for k, v in zip(names, packed + (lo_b, hi_b)):
        assert bytes(bufs[k].payload.cpu().numpy()) == v.tobytes(), k                               # the inputs are inputs
    want = CR.cut_numpy(*packed, thr, lo_b, hi_b)
    for buf, w in zip((labels, clusters, bad), want):
        assert np.array_equal(buf.view(torch.int32).cpu().numpy(), w), buf.name
    assert not want[2].any()


# ------------------------------------------------------------------ 3. every cause of `bad`

def _break(kind, log, n):
    """The log of a recording of n rows, broken in one way -> (log, min, max) of that recording."""
    lo, hi, key = (a.copy() for a in log)
    lo_b, hi_b = 1, n
    at = len(key) // 2
    if kind == "lo_equals_hi":
        lo[at] = hi[at]
    elif kind == "lo_above_hi":
        lo[at], hi[at] = hi[at], lo[at]
    elif kind == "index_of_n":
        hi[at] = n
    elif kind == "index_far_out":
        hi[at] = 2 ** 31 - 1
    elif kind == "negative_index":
        lo[at] = -1
    elif kind == "nan_key":
        key[at] = np.nan
    elif kind == "inf_key":
        key[0] = np.inf
    elif kind == "minus_inf_key":
        key[-1] = -np.inf
    elif kind == "log_too_short":
        lo, hi, key, hi_b = lo[:at], hi[:at], key[:at], 2
    elif kind == "min_above_max":
        lo_b, hi_b = 5, 4
    elif kind == "min_below_one":
        lo_b = 0
    elif kind == "more_merges_than_rows":
        lo, hi, key = (np.concatenate([a, a[-1:]]) for a in (lo, hi, key))
    elif kind == "two_parents":
        # the row a merge absorbs is absorbed again, by another row: both merges get the highest keys, so both are applied
        t = int(np.flatnonzero(hi >= 2)[0])
        u = (t + 1) % len(key)
        lo[u], hi[u] = (0 if lo[t] != 0 else 1), hi[t]
        key[t], key[u] = 3.0, 2.5
    else:
        raise ValueError(kind)
    return (lo, hi, key), lo_b, hi_b


CAUSES = ("lo_equals_hi", "lo_above_hi", "index_of_n", "index_far_out", "negative_index", "nan_key", "inf_key", "minus_inf_key", "log_too_short",
          "min_above_max", "min_below_one", "more_merges_than_rows", "two_parents")


@pytest.mark.parametrize("kind", CAUSES)
def test_a_broken_recording_is_reported_and_the_others_are_not_touched(kind):
    """Refusals by value: every index is compared with its range before it becomes an address.  The broken recording is once a small
    one and once one of several tiles; its neighbours keep the labels they get without it."""
    for sizes in ((17, 64, 129), (64, 1000, 17)):
        logs = [_log(n, 5) for n in sizes]
        clean = CR.cut_numpy(*CR.pack(logs, sizes), 0.25, [1] * 3, list(sizes))
        logs[1], lo_b, hi_b = _break(kind, logs[1], sizes[1])
        labels, clusters, bad = _check(logs, sizes, 0.25, [1, lo_b, 1], [sizes[0], hi_b, sizes[2]])
        assert bad[0] == 0 and bad[1] != 0 and bad[2] == 0, (kind, sizes, bad)
        a, b = sizes[0], sizes[0] + sizes[1]
        assert (labels[a:b] == -1).all() and clusters[1] == 0
        assert np.array_equal(labels[:a], clean[0][:a]) and np.array_equal(labels[b:], clean[0][b:]) and clusters[0] == clean[1][0]


@pytest.mark.parametrize("which", ["first_merge", "first_row"])
def test_a_broken_promise_makes_every_recording_bad(which):
    sizes = (17, 64, 129, 3)
    logs = [_log(n, 5) for n in sizes]
    # (the end of first_row is where the binding reads the number of rows from, so only first_merge can end early)
    for how in ("decreases", "starts_late") + (("ends_early",) if which == "first_merge" else ()):
        lo, hi, key, fm, fr = CR.pack(logs, sizes)
        table = fm if which == "first_merge" else fr
        if how == "decreases":
            table[2] = table[1] - 1
        elif how == "starts_late":
            table[0] = 1
        else:
            table[-1] -= 1
        labels, clusters, bad = _run((lo, hi, key, fm, fr), 0.25, [1] * 4, list(sizes))
        assert bad.all() and not clusters.any() and (labels == -1).all() and len(labels) == int(fr[-1]), (which, how)


# ------------------------------------------------------------------ 4. the drivers

@pytest.fixture(scope="module")
def recordings():
    recs = CR.driver_recordings()
    X = torch.from_numpy(np.concatenate([x for _, x in recs])).to(DEV)
    return recs, X, [len(x) for _, x in recs]


def _drive(recordings, case):
    recs, X, sizes = recordings
    thr, lo_b, hi_b = case
    with L.expect_launches(exactly={KERNEL}) as log:
        labels, info = ahc_gpu.ahc_cosine_groups(X, sizes, thr, min_clusters=lo_b, max_clusters=hi_b, return_info=True)
    assert log[KERNEL] == 1                                             # one launch of the cut for all recordings
    return labels, info


@pytest.mark.parametrize("k", CR.K_RANGE)
def test_a_known_count_equals_the_oracle(recordings, k):
    """min = max = k on the three families (400, 700 and 1000 rows; at 0.3 the threshold leaves 2, 294 and 671 clusters) with the tiny
    recordings between them, against scipy's average linkage cut into k.  A (recording, k) is left out only when the two heights on
    either side of its cut are closer than 1e-4: that is (1000 rows, k = 6) and no other."""
    labels, info = _drive(recordings, (0.3, k, k))
    skipped = CR.check_driver_case(labels, (0.3, k, k), recordings[0])
    assert skipped == ([(1000, 6)] if k == 6 else []), skipped
    fams = [f for f, _ in recordings[0]]
    assert [info["threshold_clusters"][fams.index(f)] for f in (400, 700, 1000)] == [2, 294, 671]
    assert [info["clusters"][fams.index(f)] for f in (400, 700, 1000)] == [k] * 3 and info["rounds_full"] > 0


@pytest.mark.parametrize("case", CR.DRIVER_CASES[len(CR.K_RANGE):], ids=str)
def test_a_range_equals_the_oracle(recordings, case):
    """(2, 6) at 0.3 binds at the maximum for 700 and 1000 rows, at 0.1 and 0.0 the thresholds' own counts lie inside; (4, 6) binds at
    the minimum for 400 rows."""
    labels, info = _drive(recordings, case)
    skipped = CR.check_driver_case(labels, case, recordings[0])
    assert set(skipped) <= {(1000, 6)}, skipped
    fams = [f for f, _ in recordings[0]]
    for f in (400, 700, 1000):
        assert case[1] <= info["clusters"][fams.index(f)] <= case[2], (f, info["clusters"])
    if case == (0.3, 4, 6):
        assert info["threshold_clusters"][fams.index(400)] == 2 and info["clusters"][fams.index(400)] == 4


@pytest.mark.parametrize("thr", AG.DRIVER_THRESHOLDS)
def test_bounds_that_do_not_bind_equal_the_unbounded_driver(thr):
    recs = AG.driver_recordings(thr)
    sizes = [len(x) for _, x in recs]
    X = torch.from_numpy(np.concatenate([x for _, x in recs])).to(DEV)
    with L.launches() as log:
        want, winfo = ahc_gpu.ahc_cosine_groups(X, sizes, thr, return_info=True)
    assert KERNEL not in log                                            # without bounds nothing new is launched
    with L.expect_launches(exactly={KERNEL}):
        got, info = ahc_gpu.ahc_cosine_groups(X, sizes, thr, min_clusters=1, max_clusters=[max(s, 1) for s in sizes], return_info=True)
    assert all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))
    assert info["rounds"] == winfo["rounds"] and info["clusters"] == winfo["clusters"] and info["rounds_full"] == 0
    assert info["gram_tiles"] == winfo["gram_tiles"]
    with L.expect_launches(exactly={KERNEL}):
        for i, w in enumerate(want):                                    # and each recording alone, through the rows driver
            if sizes[i] >= 2:
                a = sum(sizes[:i])
                alone = ahc_gpu.ahc_cosine_rows(X[a:a + sizes[i]], thr, min_clusters=1, max_clusters=sizes[i])
                assert np.array_equal(alone, w), i


# ------------------------------------------------------------------ 5. the pipeline

@pytest.fixture()
def small_encoder():
    """The small seeded encoder of tests/test_gpu_ahc_grouped.py."""
    from speech_diarization_amd import ecapa_annote, speech_encode, synth
    enc = speech_encode.HipEcapaEncoder(synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(128)), DEV)
    speech_encode.using_ecapa_encoder.cache_clear()
    orig = speech_encode.using_ecapa_encoder
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = lambda device="cuda": enc
    yield enc
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = orig


def test_diarize_audios_with_speaker_bounds_equals_one_recording_at_a_time(small_encoder, tmp_path):
    """A: 60 s, 2 voices (the threshold 0.70 leaves 2 speakers: tests/test_gpu_ahc_grouped.py).  B: 40 s, 3 voices (3 speakers).  D: 1.2 s,
    one window.  With min_speakers = 3, max_speakers = 6 the threshold's count of A lies outside the bounds and its bounded count
    inside; B is untouched; D has one window and one speaker whatever the bounds.  The cut of A into 3 is conditioned first: the two
    heights on either side of it are further apart than CUT_MARGIN."""
    from speech_diarization_amd import audio_io, cluster, diarization_baseline as db, synth
    import ahc_ref as A
    thr = 0.70
    conv_a, conv_b = synth.synthetic_conversation(60.0, 2, seed=0), synth.synthetic_conversation(40.0, 3, seed=1)
    speech_a = db._speech_regions(conv_a.wav.astype(np.float32), conv_a.sr, 0.35, 0.1)
    a0 = int(round(speech_a[0][0] * conv_a.sr))
    waves = {"a": conv_a.wav, "b": conv_b.wav, "d": conv_a.wav[a0:a0 + int(1.2 * 16000)]}
    wavs = []
    for name, w in waves.items():
        wavs.append(tmp_path / f"{name}.wav")
        audio_io.write_wav16(wavs[-1], w, 16000)
    speakers = lambda det: len(set(det["labels"].tolist()))  # noqa: E731
    with L.launches() as log:
        plain = [db.diarize_audio(w, 0.35, 0.1, 3, 6, clustering="ahc_gpu", clustering_threshold=thr, return_details=True) for w in wavs]
    assert KERNEL not in log and [speakers(det) for _, det in plain] == [2, 3, 1]          # without the keyword the bounds are ignored, as before
    with L.expect_launches(exactly={KERNEL}) as log:
        alone = [db.diarize_audio(w, 0.35, 0.1, 3, 6, rttm_filepath=w.with_suffix(".alone.rttm"), clustering="ahc_gpu", clustering_threshold=thr,
                                  return_details=True, speaker_bounds=True) for w in wavs]
    assert log[KERNEL] == 2                                             # D returns before any clustering
    print("speakers without bounds", [speakers(det) for _, det in plain], "with bounds", [speakers(det) for _, det in alone])
    Z = CR.host_linkage(cluster.center(alone[0][1]["embeddings"]))
    print(f"recording a: gap of the cut into 3: {CR.cut_gap(Z, 3):.4f}")
    assert CR.cut_gap(Z, 3) > A.CUT_MARGIN
    assert [speakers(det) for _, det in alone] == [3, 3, 1]
    assert np.array_equal(alone[1][1]["labels"], plain[1][1]["labels"]) and alone[1][0] == plain[1][0]
    with L.expect_launches(exactly={KERNEL}) as log:
        many = db.diarize_audios(wavs, 0.35, 0.1, 3, 6, rttm_filepaths=[w.with_suffix(".many.rttm") for w in wavs], clustering_threshold=thr,
                                 return_details=True, speaker_bounds=True)
    assert log[KERNEL] == 1
    for name, w, (seg_1, det_1), (seg_m, det_m) in zip(waves, wavs, alone, many):
        assert seg_m == seg_1 and np.array_equal(det_m["labels"], det_1["labels"]), name
        assert w.with_suffix(".many.rttm").read_bytes() == w.with_suffix(".alone.rttm").read_bytes(), name
    hp = db.DiarizationParameters(min_speakers=3, max_speakers=6, clustering_threshold=thr)
    diarizer = db.Diarizer(hp, clustering="ahc_gpu", speaker_bounds=True)
    assert diarizer.diarize_many(wavs) == [diarizer.diarize(w, None) for w in wavs]
