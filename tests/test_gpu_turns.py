"""The device speaker turns on the MI355X (include/sd_hip_turns.h: sd_turns_grouped; turns_gpu.py; turns="device" on diarize_audio,
diarize_audios and Diarizer): the entry against the numpy statement (tests/helpers/turns_ref.py), integer for integer and slot for
slot (the slots the entry leaves alone keep their poison); guard bands at exactly the sizes the header names; every cause of `bad`
and every refusal; and the public routes against the host route.  Every launch runs under the launch log, held to the label of the
path it must take, and twice."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import guarded as G  # noqa: E402
import turns_ref as T  # noqa: E402
from launch_log import expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu

LDS, WS = {"turns_kernel/lds"}, {"turns_kernel/ws"}
OUTPUTS = ("new_labels", "run_region", "run_first", "run_end", "run_label", "n_runs", "bad")
ONE = 1.0 / 16000


@pytest.fixture(scope="module")
def dev():
    from speech_diarization_amd import _native as N
    N.load()
    return torch.device("cuda")


def _word(poison: int) -> int:
    return int(np.frombuffer(bytes([poison] * 4), np.int32)[0])


def _run(dev, tables, frame_s=0.01, poison=0xFF, label=None):
    """One call of the entry on guarded buffers of exactly the sizes the header names -> dict of numpy arrays.  `tables`: the seven
    tables of `turns_ref.tables_of`; `label`: the launch label the call must be logged under (default: by the window count)."""
    from speech_diarization_amd import _native as N
    from speech_diarization_amd import ops
    fw, fr, rfw, centre, start, frames, labels = tables
    ng, nr, nw = len(fw) - 1, len(rfw) - 1, len(labels)
    assert len(fr) == ng + 1 and len(centre) == nw and len(start) == len(frames) == nr
    ins = [G.guarded_from(torch.from_numpy(np.ascontiguousarray(t, dt)), dev, name) for name, t, dt in (
        ("first_window", fw, np.int32), ("first_region", fr, np.int32), ("region_first_window", rfw, np.int32), ("centre", centre, np.float64),
        ("region_start", start, np.float64), ("n_frames", frames, np.int32), ("labels", labels, np.int32))]
    before = [b.payload.cpu().numpy().tobytes() for b in ins]
    outs = {name: G.guarded(4 * (ng if name in ("n_runs", "bad") else nw), poison, dev, name) for name in OUTPUTS}
    need = int(N.load().sd_turns_workspace_bytes(nw, ng))
    assert need == (8 * nw if nw > T.LDS_WINDOWS else 0)
    ws = G.guarded(need, poison, dev, "ws")
    label = (WS if need else LDS) if label is None else label
    t_fw, t_fr, t_rfw, t_centre, t_start, t_frames, t_labels = ins
    with expect_launches(exactly=label) as log:
        ops.launch("sd_turns_grouped", ws.raw, t_fw.ptr, t_fr.ptr, ng, t_rfw.ptr, nr, t_centre.ptr, nw, t_start.ptr, t_frames.ptr, C.c_double(frame_s),
                   t_labels.ptr, outs["new_labels"].ptr, outs["n_runs"].ptr, outs["run_region"].ptr, outs["run_first"].ptr, outs["run_end"].ptr,
                   outs["run_label"].ptr, outs["bad"].ptr, ws.ptr, need)
        torch.cuda.synchronize()
    assert log == {next(iter(label)): 1}
    G.assert_guards_intact(ws, *ins, *outs.values())
    assert [b.payload.cpu().numpy().tobytes() for b in ins] == before                            # the inputs are only read
    return {name: b.view(torch.int32).cpu().numpy().copy() for name, b in outs.items()}


def _run_twice(dev, tables, frame_s=0.01, label=None):
    """Two launches, a different poison under the outputs each time, each equal to the statement in EVERY slot: what the entry writes
    is the statement's, what it leaves alone still holds the poison -> the results of the first, and the statement"""
    first = want = None
    for poison in G.POISONS[:2]:
        got = _run(dev, tables, frame_s, poison, label)
        ref = T.turns_entry(*tables[:6], frame_s, tables[6], fill=_word(poison))
        for name in OUTPUTS:
            assert np.array_equal(got[name], ref[name]), (name, np.flatnonzero(got[name] != ref[name])[:8], got[name][:12], ref[name][:12])
        if first is None:
            first, want = got, ref
    return first, want


def _check(dev, recordings, frame_s=0.01, label=None):
    """`_run_twice` on the launch of `recordings` ([(rfw, centre, region_start, n_frames, labels)]) -> (got, want, tables)"""
    tables = T.tables_of(recordings)
    got, want = _run_twice(dev, tables, frame_s, label)
    return got, want, tables


# ------------------------------------------------------------------ the smallest shapes

def test_one_window_one_frame_and_a_window_without_a_frame(dev):
    """One recording, one region, one window, one frame; and a region of two windows whose second lies past the last frame's midpoint"""
    got, _, _ = _check(dev, [T.even_recording([1], [0], hop=0.01)], label=LDS)
    assert got["n_runs"].tolist() == [1] and [got[k][0] for k in OUTPUTS[:5]] == [0, 0, 0, 1, 0] and got["bad"].tolist() == [0]
    two = (np.array([0, 2]), np.array([1.1, 1.3]), np.array([1.0]), np.array([20]), np.array([1, 0]))     # the midpoint 1.2 is past frame 19 at 1.195
    got, _, _ = _check(dev, [two], label=LDS)
    assert got["n_runs"].tolist() == [1] and got["new_labels"].tolist() == [0, 1] and got["run_end"][0] == 20 and got["run_label"][0] == 0
    two = (np.array([0, 2]), np.array([1.1, 1.28]), np.array([1.0]), np.array([20]), np.array([1, 0]))    # the midpoint 1.19: frame 19 goes to the second
    got, _, _ = _check(dev, [two], label=LDS)
    assert got["n_runs"].tolist() == [2] and got["run_first"].tolist() == [0, 19] and got["run_end"].tolist() == [19, 20]


def test_regions_across_the_pass_boundary(dev):
    """Regions of 255, 256, 257 and 513 windows in one recording, and each alone: the carries of both scans cross a step of 256"""
    rs = np.random.RandomState(0)
    counts = [255, 256, 257, 513]
    n = sum(counts)
    for labels in (np.repeat(rs.randint(0, 4, n), 3)[:n], rs.randint(-1, 3, n), np.arange(n) % 2):
        got, _, _ = _check(dev, [T.even_recording(counts, labels)], label=LDS)
        assert got["n_runs"][0] >= 4
    alone = [T.even_recording([c], np.arange(c) // 5 % 3) for c in counts]
    got, _, tables = _check(dev, alone, label=LDS)
    assert got["n_runs"].tolist() == [(c + 4) // 5 for c in counts]


def test_a_window_without_a_frame_at_the_pass_boundary(dev):
    """Three centres a sample apart at windows 254-256, then at 255-257: window 255, then window 256, owns no frame, and the runs on
    both sides of the step of 256 are the statement's; alternating labels, so that every owner is a head"""
    for at in (255, 256):
        rfw, centre, start, frames, labels = T.even_recording([300], np.arange(300) % 2)
        centre[at] = centre[at - 1] + ONE
        centre[at + 1] = centre[at - 1] + 2 * ONE
        f, _ = T.first_frames(rfw, centre, start, frames, 0.01)
        assert f[at] == f[at + 1] and f[at - 1] < f[at] and f[at + 1] < f[at + 2]                # `at` owns nothing, its neighbours do
        got, _, _ = _check(dev, [(rfw, centre, start, frames, labels)], label=LDS)
        assert got["n_runs"].tolist() == [298]             # 299 owners; the two beside `at` carry one label and meet in one run
        same = labels.copy()
        same[at - 2:at + 3] = 1                          # and with equal labels around it, one run spans the step
        got, _, _ = _check(dev, [(rfw, centre, start, frames, same)], label=LDS)
        assert got["n_runs"][0] in (294, 296)              # the five merge, and at 256 also with both neighbours


def test_a_label_first_seen_in_the_second_pass(dev):
    labels = np.zeros(600, np.int64)
    labels[[300, 301, 302, 599]] = [7, 3, 7, 5]
    labels[10] = 9
    got, _, _ = _check(dev, [T.even_recording([600], labels), T.even_recording([40, 300], np.r_[np.full(300, 339), np.arange(40)[::-1]])], label=LDS)
    assert got["new_labels"][[0, 10, 300, 301, 302, 599]].tolist() == [0, 1, 2, 3, 2, 4]
    assert got["new_labels"][600:604].tolist() == [0, 0, 0, 0] and got["new_labels"][900:903].tolist() == [1, 2, 3]


# ------------------------------------------------------------------ labels

def test_equal_alternating_and_noise_labels(dev):
    """All labels equal: one run per region that has windows.  Strictly alternating: as many runs as windows, the capacity exactly.
    -1 mixed in: it is a label of its own"""
    counts = [30, 0, 1, 270, 7]
    n = sum(counts)
    got, _, _ = _check(dev, [T.even_recording(counts, np.full(n, 5))], label=LDS)
    assert got["n_runs"].tolist() == [4] and got["run_region"][:4].tolist() == [0, 2, 3, 4] and (got["new_labels"] == 0).all()
    got, _, _ = _check(dev, [T.even_recording(counts, np.arange(n) % 2), T.even_recording([3], [0, 0, 0])], label=LDS)
    assert got["n_runs"].tolist() == [n, 1] and (got["run_region"][:n] >= 0).all()                 # the slice is full: no slot is left
    noise = np.where(np.arange(n) % 3 == 0, -1, np.arange(n) % 2)
    got, _, _ = _check(dev, [T.even_recording(counts, noise)], label=LDS)
    assert (got["new_labels"][::3] == -1).all() and -1 in got["run_label"][:got["n_runs"][0]].tolist()


# ------------------------------------------------------------------ the size of the tables

@pytest.mark.parametrize("n,label", [(T.LDS_WINDOWS - 1, LDS), (T.LDS_WINDOWS, LDS), (T.LDS_WINDOWS + 1, WS)])
def test_recordings_around_the_size_of_the_lds_tables(dev, n, label):
    """One window below, at and above SD_TURNS_LDS_WINDOWS: the first two launches need no workspace and are labelled so, the third
    keeps its tables in the workspace; labels that visit most of [0, n)"""
    rs = np.random.RandomState(n)
    counts = [97] * (n // 97) + [n % 97]
    labels = np.repeat(rs.permutation(n)[:n // 2 + 1], 2)[:n]
    labels[-1] = n - 1
    got, _, _ = _check(dev, [T.even_recording(counts, labels)], label=label)
    assert got["n_runs"][0] > n // 3 and got["new_labels"].max() >= n // 2 - 1


def test_a_large_launch_of_small_recordings_and_a_large_recording_beside_a_small_one(dev):
    """More than SD_TURNS_LDS_WINDOWS windows in all: the launch takes a workspace (and the label says so) whether or not a recording
    uses it"""
    rs = np.random.RandomState(3)
    small = [T.even_recording([100, 60], rs.randint(0, 3, 160)) for _ in range(27)]
    got, _, _ = _check(dev, small, label=WS)
    assert len(small) * 160 > T.LDS_WINDOWS and got["n_runs"].min() >= 2
    n = T.LDS_WINDOWS + 5
    mixed = [T.even_recording([50], rs.randint(0, 50, 50)), T.even_recording([n], rs.randint(-1, n, n)), T.even_recording([9], np.arange(9))]
    got, _, _ = _check(dev, mixed, label=WS)
    assert got["n_runs"][2] == 9


# ------------------------------------------------------------------ folders, an hour-long region, the same bytes twice

def test_a_random_folder_equals_the_statement(dev):
    """40 recordings of 0-600 windows; recordings 5 and 17 have no windows (17 has two regions), and regions in the middle have none"""
    recs = T.random_folder()
    assert len(recs) == 40 and len(recs[5][1]) == 0 and len(recs[17][1]) == 0 and len(recs[17][2]) == 2
    assert any(np.any(np.diff(r[0]) == 0) and len(r[1]) for r in recs)
    got, _, _ = _check(dev, recs)
    assert got["n_runs"][5] == 0 and got["n_runs"][17] == 0 and (got["n_runs"] > 0).sum() >= 30 and not got["bad"].any()


def test_an_hour_long_region_of_three_windows(dev):
    """360 000 frames, three windows: the cost follows the windows (19 steps of a binary search), not the frames"""
    hour = (np.array([0, 3]), np.array([600.0, 1800.0, 3000.0]), np.array([0.0]), np.array([360000]), np.array([2, 1, 2]))
    got, _, _ = _check(dev, [hour], label=LDS)
    assert got["n_runs"].tolist() == [3] and got["run_first"].tolist() == [0, 120000, 240000] and got["run_end"].tolist() == [120000, 240000, 360000]
    assert got["run_label"].tolist() == [0, 1, 0]


def test_two_launches_give_the_same_bytes(dev):
    tables = T.tables_of(T.random_folder(seed=1, n_recordings=12))
    a, b = _run(dev, tables, poison=0x7B), _run(dev, tables, poison=0x7B)
    assert all(a[name].tobytes() == b[name].tobytes() for name in OUTPUTS) and a["n_runs"].sum() > 100


# ------------------------------------------------------------------ flags and refusals

def test_every_cause_of_bad(dev):
    """A label that is not below the recording's window count, and a broken promise of the recording's own (its slice of
    region_first_window, a frame count, its centres): that recording alone, its slices untouched.  first_window or first_region
    broken anywhere: every recording, nothing written but the two words of each"""
    rs = np.random.RandomState(4)
    recs = [T.even_recording([12, 30], rs.randint(0, 3, 42)), T.even_recording([300], rs.randint(-1, 4, 300)), T.even_recording([], []),
            T.even_recording([5, 0, 5], rs.randint(0, 2, 10))]
    fw, fr, rfw, centre, start, frames, labels = T.tables_of(recs)

    def launch(**change):
        t = dict(fw=fw, fr=fr, rfw=rfw, centre=centre, start=start, frames=frames, labels=labels)
        for name, (at, value) in change.items():
            t[name] = t[name].copy()
            t[name][at] = value
        return _run_twice(dev, tuple(t.values()), label=LDS)[0]
    assert not launch()["bad"].any()
    for at, value, who in ((0, 42, 0), (41, 10 ** 9, 0), (42 + 299, 300, 1), (342 + 9, 10, 3)):
        got = launch(labels=(at, value))
        assert got["bad"].tolist() == [T.BAD_LABEL * (g == who) for g in range(4)] and got["n_runs"][who] == 0, (at, value)
        assert (got["new_labels"][fw[who]:fw[who + 1]] == -1).all() and (np.delete(got["n_runs"], [2, who]) > 0).all()
    own = [dict(rfw=(1, -3)), dict(rfw=(1, 43)), dict(rfw=(0, 1)), dict(rfw=(2, 41)), dict(rfw=(2, 10 ** 6))]       # recordings 0, 0, 0, 0 and 1, 0 and 1
    assert [launch(**c)["bad"].tolist() for c in own] == [[2, 0, 0, 0], [2, 0, 0, 0], [2, 0, 0, 0], [2, 2, 0, 0], [2, 2, 0, 0]]
    own = [dict(frames=(2, 0)), dict(frames=(4, -5)), dict(centre=(50, centre[49])), dict(centre=(60, np.nan)), dict(centre=(342, np.inf)),
           dict(start=(5, np.nan)), dict(centre=(343, centre[342] + 2.0 ** -45))]
    assert [launch(**c)["bad"].tolist() for c in own] == [[0, 2, 0, 0], [0, 0, 0, 2], [0, 2, 0, 0], [0, 2, 0, 0], [0, 0, 0, 2], [0, 0, 0, 2], [0, 0, 0, 2]]
    assert launch(labels=(0, 42), centre=(10, centre[9]))["bad"].tolist() == [T.BAD_LABEL + T.BAD_PROMISE, 0, 0, 0]
    for change in (dict(fw=(0, 1)), dict(fw=(2, 41)), dict(fw=(4, 351)), dict(fw=(4, 353)), dict(fw=(1, -1)), dict(fr=(0, 1)), dict(fr=(2, 1)),
                   dict(fr=(4, 7)), dict(fr=(3, 10 ** 6))):
        got = launch(**change)
        assert got["bad"].tolist() == [T.BAD_PROMISE] * 4 and not got["n_runs"].any(), change
        assert all((got[name] == -1).all() for name in OUTPUTS[:5])                                # every slice keeps its poison


def test_every_refusal_comes_before_any_launch(dev):
    """Every SD_ERR_* of the header through the entry on real buffers: the status, and no launch in the log"""
    from speech_diarization_amd import _native as N
    lib = N.load()
    n = T.LDS_WINDOWS + 8
    ints = torch.zeros((8 * n,), dtype=torch.int32, device=dev)
    dbl = torch.zeros((2 * n,), dtype=torch.float64, device=dev)
    ws = torch.zeros((8 * n + 16,), dtype=torch.uint8, device=dev)
    at = lambda k: ints.data_ptr() + 4 * n * k           # noqa: E731
    good = dict(first_window=at(0), first_region=at(0) + 64, n_recordings=4, region_first_window=at(0) + 128, n_regions=6, centre=dbl.data_ptr(),
                n_windows=n, region_start=dbl.data_ptr() + 8 * n, n_frames=at(0) + 256, frame_s=0.01, labels=at(1), new_labels=at(2), n_runs=at(0) + 512,
                run_region=at(3), run_first=at(4), run_end=at(5), run_label=at(6), bad=at(7), ws=ws.data_ptr(), ws_bytes=8 * n)
    cases = [(dict(n_recordings=0), -1), (dict(n_recordings=-1), -1), (dict(n_windows=-1), -1), (dict(n_regions=-1), -1), (dict(frame_s=0.0), -1),
             (dict(frame_s=-0.01), -1), (dict(frame_s=float("nan")), -1), (dict(frame_s=float("inf")), -1), (dict(ws=ws.data_ptr() + 4), -1),
             (dict(ws_bytes=8 * n - 1), -3), (dict(ws_bytes=0), -3)]
    cases += [({name: None}, -1) for name, value in good.items() if name not in ("n_recordings", "n_regions", "n_windows", "frame_s", "ws_bytes")]
    assert len(cases) == 11 + 15
    with expect_launches() as log:
        for change, code in cases:
            a = dict(good, **change)
            status = lib.sd_turns_grouped(*a.values(), None)
            assert status == code and N.last_error().startswith("sd_turns_grouped: "), (change, status, N.last_error())
        torch.cuda.synchronize()
    assert not any(lb.startswith("turns_kernel") for lb in log)
    with expect_launches(exactly=WS):                    # and the same buffers are accepted: first_window all 0 with n windows breaks the promise
        assert lib.sd_turns_grouped(*good.values(), None) == 0
        torch.cuda.synchronize()
    assert ints[7 * n:7 * n + 4].tolist() == [T.BAD_PROMISE] * 4 and not ints[n:7 * n].any()


# ------------------------------------------------------------------ the routes

def _small_sd(width=128):
    from speech_diarization_amd import synth
    return synth.make_ecapa_state_dict(1234, synth.EcapaConfig.small(width))


@pytest.fixture()
def small_encoder(dev):
    """The small seeded encoder of tests/test_gpu_scd.py."""
    from speech_diarization_amd import ecapa_annote, speech_encode
    enc = speech_encode.HipEcapaEncoder(_small_sd(), dev)
    speech_encode.using_ecapa_encoder.cache_clear()
    orig = speech_encode.using_ecapa_encoder
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = lambda device="cuda": enc
    yield enc
    speech_encode.using_ecapa_encoder = ecapa_annote.using_ecapa_encoder = orig


def _audios():
    from speech_diarization_amd import synth
    ys = [synth.synthetic_conversation(12.0, 2, seed=0).wav.astype(np.float32), np.zeros(3 * 16000, np.float32),
          synth.synthetic_conversation(8.0, 3, seed=1).wav.astype(np.float32)]
    return [{"waveform": y, "sample_rate": 16000, "uri": f"rec{i}"} for i, y in enumerate(ys)]


def _same(host, device, paths=None):
    for i, ((seg_h, det_h), (seg_d, det_d)) in enumerate(zip(host, device)):
        assert seg_d == seg_h and np.array_equal(det_d["labels"], det_h["labels"]) and det_d["labels"].dtype == det_h["labels"].dtype, i
        if paths:
            assert paths["device"][i].read_bytes() == paths["host"][i].read_bytes(), i


def test_diarize_audios_with_the_device_turns_equals_the_host_route(dev, small_encoder, tmp_path):
    """Three short recordings, one of them silent: segments, `details["labels"]` and RTTM bytes, with ONE turns launch for the folder;
    and the same beside vad="device" and beside speaker_bounds=True"""
    from speech_diarization_amd import diarization_baseline as db
    audios = _audios()
    for kw in ({}, {"vad": "device"}, {"speaker_bounds": True}):
        paths = {route: [tmp_path / f"{route}{len(kw)}{i}.rttm" for i in range(3)] for route in ("host", "device")}
        host = db.diarize_audios(audios, 0.35, 0.1, 2, 6, rttm_filepaths=paths["host"], return_details=True, **kw)
        with expect_launches(exactly=LDS) as log:
            device = db.diarize_audios(audios, 0.35, 0.1, 2, 6, rttm_filepaths=paths["device"], return_details=True, turns="device", **kw)
        assert log["turns_kernel/lds"] == 1
        _same(host, device, paths)
        assert host[1][0] == [] and len(host[0][0]) and len(host[2][0])
    with expect_launches() as log:
        assert db.diarize_audios([audios[1]], 0.35, 0.1, 2, 6, turns="device") == [[]]             # no windows at all: nothing to launch
        with pytest.raises(ValueError, match="turns must be 'host' or 'device'"):
            db.diarize_audios(audios, 0.35, 0.1, 2, 6, turns="gpu")
    assert not any(lb.startswith("turns_kernel") for lb in log)


def test_diarize_audio_and_the_diarizer_with_the_device_turns(dev, small_encoder, tmp_path):
    """`diarize_audio(turns="device")` equals its default for clustering="ahc_gpu" and "ahc"; `Diarizer(turns="device")` gives the
    same segments from `diarize` and the same RTTM files from `diarize_many`"""
    from speech_diarization_amd import diarization_baseline as db
    audios = _audios()
    for clustering in ("ahc_gpu", "ahc"):
        for audio in audios[:2]:
            host = db.diarize_audio(audio, 0.35, 0.1, 2, 6, clustering=clustering, return_details=True)
            with expect_launches(at_least=LDS if host[0] else ()) as log:
                device = db.diarize_audio(audio, 0.35, 0.1, 2, 6, clustering=clustering, return_details=True, turns="device")
            _same([host], [device])
            assert log.get("turns_kernel/lds", 0) == (1 if host[0] else 0)
    with pytest.raises(ValueError, match="turns must be 'host' or 'device'"):
        db.diarize_audio(audios[0], 0.35, 0.1, 2, 6, turns="gpu")
    hp = db.DiarizationParameters()
    paths = {route: [tmp_path / f"many_{route}{i}.rttm" for i in range(3)] for route in ("host", "device")}
    host = db.Diarizer(hp, clustering="ahc_gpu").diarize_many(audios, paths["host"])
    with expect_launches(exactly=LDS) as log:
        device = db.Diarizer(hp, clustering="ahc_gpu", turns="device").diarize_many(audios, paths["device"])
    assert log["turns_kernel/lds"] == 1 and device == host and len(host[0])
    assert [p.read_bytes() for p in paths["device"]] == [p.read_bytes() for p in paths["host"]]
    with expect_launches(exactly=LDS):
        assert db.Diarizer(hp, clustering="ahc_gpu", turns="device").diarize(audios[0], None) == db.Diarizer(hp, clustering="ahc_gpu").diarize(audios[0], None)
