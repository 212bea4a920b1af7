"""The device VAD on the MI355X (include/sd_hip_vad.h: sd_vad_energy_grouped_f32, sd_vad_segments_grouped; vad_gpu.py; vad="device" on
diarize_audio, diarize_audios and Diarizer): entry 2 integer for integer against the numpy statement for recordings of every critical
size in one launch, the stages pinned one at a time, guard bands at exact buffer sizes, every cause of `bad`; entry 1 against the
float64 statement under a bar made of the host scorer's own distance from it; and the public routes against the host chain.  Every
launch runs under the launch log, held to its kernel, and twice with identical bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import guarded as G  # noqa: E402
import vad_ref as V  # noqa: E402
from launch_log import expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu

ENERGY_KERNEL = {"vad_energy_kernel"}
SEGMENTS_KERNEL = {"vad_segments_kernel"}
KERNELS = ENERGY_KERNEL | SEGMENTS_KERNEL


@pytest.fixture(scope="module")
def dev():
    from speech_diarization_amd import _native as N
    N.load()
    return torch.device("cuda")


def _fill(poison: int) -> int:
    return int(np.frombuffer(bytes([poison] * 4), np.int32)[0])


# ------------------------------------------------------------------ entry 2

def _segments(dev, recs, prm, on=0.6, off=0.4, first_frame=None, first_seg=None, want_mask=True, poison=0xFF):
    """One call of the entry on guarded buffers of exactly the sizes the header names -> (n_segs, seg_start, seg_end, mask, bad) as
    numpy.  `recs`: one f32 probability vector per recording; the tables default to the ones the driver would make."""
    from speech_diarization_amd import _native as N
    from speech_diarization_amd import ops
    counts = np.array([len(p) for p in recs])
    ff = np.concatenate([[0], np.cumsum(counts)]) if first_frame is None else np.asarray(first_frame)
    fs = np.concatenate([[0], np.cumsum((counts + 1) // 2)]) if first_seg is None else np.asarray(first_seg)
    ng, n_frames, cap = len(recs), int(counts.sum()), int(fs[-1])
    flat = np.concatenate(recs).astype(np.float32)
    probs = G.guarded_from(torch.from_numpy(flat), dev, "probs")
    t_ff = G.guarded_from(torch.from_numpy(ff.astype(np.int32)), dev, "first_frame")
    t_fs = G.guarded_from(torch.from_numpy(fs.astype(np.int32)), dev, "first_seg")
    n_segs, bad = (G.guarded(4 * ng, poison, dev, name) for name in ("n_segs", "bad"))
    seg_start, seg_end = (G.guarded(4 * cap, poison, dev, name) for name in ("seg_start", "seg_end"))
    mask = G.guarded(n_frames, poison, dev, "mask")
    need = int(N.load().sd_vad_segments_workspace_bytes(cap, ng))
    assert need == 8 * cap
    ws = G.guarded(need, poison, dev, "ws")
    bufs = (probs, t_ff, t_fs, n_segs, bad, seg_start, seg_end, mask, ws)
    with expect_launches(exactly=SEGMENTS_KERNEL) as log:
        ops.launch("sd_vad_segments_grouped", ws.raw, probs.ptr, t_ff.ptr, ng, n_frames, C.c_float(on), C.c_float(off), *prm, t_fs.ptr, cap,
                   n_segs.ptr, seg_start.ptr, seg_end.ptr, mask.ptr if want_mask else None, bad.ptr, ws.ptr, need)
        torch.cuda.synchronize()
    assert log == {"vad_segments_kernel": 1}
    G.assert_guards_intact(*bufs)
    assert probs.view(torch.float32).cpu().numpy().tobytes() == flat.tobytes()                   # the inputs are only read
    return tuple(b.view(dt).cpu().numpy().copy() for b, dt in ((n_segs, torch.int32), (seg_start, torch.int32), (seg_end, torch.int32),
                                                              (mask, torch.uint8), (bad, torch.int32)))


def _segments_twice(dev, recs, prm, **kw):
    """Two launches, a different poison under the outputs each time -> the results of the first, the slots the entry leaves alone
    holding that poison; what it writes is identical"""
    a = _segments(dev, recs, prm, poison=G.POISONS[0], **kw)
    b = _segments(dev, recs, prm, poison=G.POISONS[1], **kw)
    for x, y, name in zip(a, b, ("n_segs", "seg_start", "seg_end", "mask", "bad")):
        if name in ("seg_start", "seg_end"):
            wrote = (x != _fill(G.POISONS[0])) | (y != _fill(G.POISONS[1]))
            assert np.array_equal(x[wrote], y[wrote]), name
        elif name != "mask" or kw.get("want_mask", True):
            assert x.tobytes() == y.tobytes(), name
    return a


def _assert_equal(got, want, what=""):
    for x, y, name in zip(got, want, ("n_segs", "seg_start", "seg_end", "mask", "bad")):
        assert x.dtype == y.dtype and np.array_equal(x, y), f"{what}{name}: {int((x != y).sum())} of {x.size} differ, first at {int(np.flatnonzero(x != y)[0])}"


SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, V.LDS_FRAMES - 1, V.LDS_FRAMES, V.LDS_FRAMES + 1, 4 * V.LDS_FRAMES + 5)
_RECS = {}


def _recordings():
    """Every probability family at every critical size, made once and shared: [(name, f32 [n])]"""
    if not _RECS:
        _RECS["all"] = [(f"{name}@{n}", p) for i, n in enumerate(SIZES) for name, p in V.prob_families(n, seed=100 + i).items()]
    return _RECS["all"]


@pytest.mark.parametrize("which", sorted(V.PARAMS))
def test_every_size_and_family_in_one_launch_equals_the_statement(dev, which):
    """135 recordings (9 families x 15 sizes: around a wave, a step of 1 024 frames, the LDS limit and several times it) in one launch,
    in two orders, per parameter set: counts, starts, ends, masks and flags, integer for integer"""
    prm, recs = V.PARAMS[which], _recordings()
    assert V.LDS_FRAMES == 16383 and max(SIZES) > 4 * V.LDS_FRAMES
    for order in (list(range(len(recs))), list(range(len(recs)))[::-1]):
        ps = [recs[i][1] for i in order]
        counts = np.array([len(p) for p in ps])
        ff, fs = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum((counts + 1) // 2)])
        want = V.segments_entry(np.concatenate(ps), ff, fs, 0.6, 0.4, *prm, seg_fill=_fill(G.POISONS[0]))
        got = _segments_twice(dev, ps, prm)
        _assert_equal(got, want, f"{which}: ")
        assert not got[4].any() and got[0].sum() > 100
    between = [i for i, (name, _) in enumerate(recs) if name.startswith("between@") or name.startswith("below@")]
    assert between and not got[0][[len(recs) - 1 - i for i in between]].any()                      # nothing from what never starts


@pytest.mark.parametrize("stage", ("open", "close", "min_run", "max_gap"))
def test_one_stage_at_a_time(dev, stage):
    """open_len = close_len = 1 with min_run = max_gap = 0 is the identity, so each stage is pinned alone, for every line length"""
    rs = np.random.RandomState(7)
    recs = [V.built_probs([L + d for L in V.LINES for d in (-1, 0, 1) if L + d > 0] * 2, lead=lead, tail=tail) for lead, tail in ((0, 0), (3, 1), (1, 7))]
    recs += [rs.uniform(0, 1, n).astype(np.float32) for n in (1, 7, 300, 1025)] + [np.repeat(rs.uniform(0, 1, 400), 3).astype(np.float32)]
    for L in V.LINES + (35,):
        prm = {"open": (L, 1, 0, 0), "close": (1, L, 0, 0), "min_run": (1, 1, L, 0), "max_gap": (1, 1, 0, L)}[stage]
        counts = np.array([len(p) for p in recs])
        ff, fs = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum((counts + 1) // 2)])
        want = V.segments_entry(np.concatenate(recs), ff, fs, 0.6, 0.4, *prm, seg_fill=_fill(G.POISONS[0]))
        _assert_equal(_segments_twice(dev, recs, prm), want, f"{stage} {L}: ")
    # the identity itself: the runs of the hysteresis mask, and the mask
    want = V.segments_entry(np.concatenate(recs), ff, fs, 0.6, 0.4, 1, 1, 0, 0, seg_fill=_fill(G.POISONS[0]))
    got = _segments_twice(dev, recs, (1, 1, 0, 0))
    _assert_equal(got, want, "identity: ")
    at = 0
    for p in recs:
        assert np.array_equal(got[3][at:at + len(p)].astype(bool), V.hysteresis_literal(p, 0.6, 0.4))
        at += len(p)


def test_other_thresholds_and_no_mask(dev):
    """Thresholds that are no round numbers in f32, values exactly on them, and the nullable mask"""
    rs = np.random.RandomState(3)
    on, off = 0.7, 0.30000001
    vals = np.array([np.float32(on), np.nextafter(np.float32(on), np.float32(0)), np.float32(off), np.nextafter(np.float32(off), np.float32(0)),
                     0.5, np.nan], np.float32)
    recs = [rs.choice(vals, n) for n in (5, 64, 1000, 2049)]
    counts = np.array([len(p) for p in recs])
    ff, fs = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum((counts + 1) // 2)])
    for prm in ((1, 1, 0, 0), (3, 2, 4, 2)):
        want = V.segments_entry(np.concatenate(recs), ff, fs, on, off, *prm, seg_fill=_fill(G.POISONS[0]))
        _assert_equal(_segments_twice(dev, recs, prm, on=on, off=off), want)
        got = _segments_twice(dev, recs, prm, on=on, off=off, want_mask=False)
        assert np.all(got[3] == G.POISONS[0])                                                   # a null mask: nothing written
        _assert_equal(got[:3] + got[4:], want[:3] + want[4:])


def test_every_cause_of_bad(dev):
    rs = np.random.RandomState(5)
    recs = [np.repeat(rs.uniform(0, 1, n // 3 + 1), 3)[:n].astype(np.float32) for n in (100, 257, 64, 1500)]
    counts = np.array([len(p) for p in recs])
    ff, fs = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum((counts + 1) // 2)])
    prm = V.PARAMS["identity"]
    flat, fill = np.concatenate(recs), _fill(G.POISONS[0])
    # a share one run too small: that recording alone (the next one gets the run, so the table keeps its promise)
    small = fs.copy()
    small[2] -= 1
    want = V.segments_entry(flat, ff, small, 0.6, 0.4, *prm, seg_fill=fill)
    assert want[4].tolist() == [0, V.BAD_CAPACITY, 0, 0]
    _assert_equal(_segments_twice(dev, recs, prm, first_seg=small), want, "capacity: ")
    # a broken promise, in either table, at either end or in the middle: every recording, nothing written but zeros
    for name, table, broken in (("first_frame", ff, [(0, 1), (2, int(ff[1]) - 1), (4, int(ff[4]) - 1), (3, int(ff[4]) + 1), (1, -1)]),
                                ("first_seg", fs, [(0, 1), (2, int(fs[1]) - 1), (3, int(fs[4]) + 1), (1, -5)])):
        for at, value in broken:
            t = table.copy()
            t[at] = value
            kw = {name: t}
            want = V.segments_entry(flat, kw.get("first_frame", ff), kw.get("first_seg", fs), 0.6, 0.4, *prm, seg_fill=fill)
            assert want[4].tolist() == [V.BAD_PROMISE] * 4 and not want[3].any() and not want[0].any()
            _assert_equal(_segments_twice(dev, recs, prm, **kw), want, f"{name}[{at}] = {value}: ")


# ------------------------------------------------------------------ entry 1

def _energy(dev, signal, first_sample, n_samples, first_frame, win, hop, thr=-35.0, slope=0.6, poison=0xFF):
    from speech_diarization_amd import ops
    ng, n_frames = len(n_samples), int(first_frame[-1])
    sig = G.guarded_from(torch.from_numpy(np.asarray(signal, np.float32)), dev, "signal")
    t_fs = G.guarded_from(torch.from_numpy(np.asarray(first_sample, np.int64)), dev, "first_sample")
    t_ns = G.guarded_from(torch.from_numpy(np.asarray(n_samples, np.int32)), dev, "n_samples")
    t_ff = G.guarded_from(torch.from_numpy(np.asarray(first_frame, np.int32)), dev, "first_frame")
    probs, bad = G.guarded(4 * n_frames, poison, dev, "probs"), G.guarded(4 * ng, poison, dev, "bad")
    with expect_launches(exactly=ENERGY_KERNEL) as log:
        ops.launch("sd_vad_energy_grouped_f32", sig.raw, sig.ptr, C.c_longlong(len(signal)), t_fs.ptr, t_ns.ptr, ng, win, hop, C.c_float(thr),
                   C.c_float(slope), t_ff.ptr, n_frames, probs.ptr, bad.ptr)
        torch.cuda.synchronize()
    assert log == {"vad_energy_kernel": 1}
    G.assert_guards_intact(sig, t_fs, t_ns, t_ff, probs, bad)
    return probs.view(torch.float32).cpu().numpy().copy(), bad.view(torch.int32).cpu().numpy().copy()


def _energy_twice(dev, *a, **kw):
    x, y = _energy(dev, *a, poison=G.POISONS[0], **kw), _energy(dev, *a, poison=G.POISONS[1], **kw)
    assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
    return x


def _pack(recs, gaps):
    """The recordings with `gaps[i]` samples of NaN in front of recording i (odd gaps: first_sample is not 16-byte aligned)"""
    parts, first_sample, at = [], [], 0
    for y, gap in zip(recs, gaps):
        parts += [np.full(gap, np.nan, np.float32), y]
        first_sample.append(at + gap)
        at += gap + len(y)
    return np.concatenate(parts), np.array(first_sample), np.array([len(y) for y in recs])


@pytest.mark.parametrize("win,hop", [(480, 160), (400, 200), (480, 480), (7, 3), (30, 7), (13001, 5)])
def test_energy_against_the_float64_statement(dev, win, hop):
    """Recordings of exactly win, win + hop - 1 and win + hop samples, 63 / 64 / 65 / 130 frames (a tile is 64), odd offsets; silence,
    full scale and a NaN sample.  (13001, 5) is read in place: 63 x 5 + 13001 floats are more than a tile stages.
    Bar: max |p - p64| <= 16 x (the host EnergyScorer's own distance from float64 on the same frames) + 2^-23."""
    from speech_diarization_amd import vad
    rs = np.random.RandomState(win + hop)
    lens = [win, win + hop - 1, win + hop, win + 62 * hop, win + 63 * hop, win + 64 * hop + hop // 2, win + 129 * hop, win + 200 * hop, win + 70 * hop,
            win + 66 * hop]
    recs = [(10 ** rs.uniform(-3.5, -0.5) * rs.standard_normal(n) * (rs.uniform(0, 1, n) < 0.7)).astype(np.float32) for n in lens]
    recs[8][:] = 0.0                                                           # silence: the clamp
    recs[9][:] = np.where(rs.uniform(0, 1, len(recs[9])) < 0.5, 1.0, -1.0)     # full scale
    nan_at = len(recs[7]) // 2 if 4 * win < len(recs[7]) else 2 * hop + 1          # inside some frames of the recording, not all
    recs[7][nan_at] = np.nan
    signal, first_sample, n_samples = _pack(recs, [1, 3, 0, 5, 2, 7, 1, 1, 3, 9])
    assert any(fs % 4 for fs in first_sample)
    counts = np.array([V.frame_count(n, win, hop) for n in n_samples])
    assert counts[:3].tolist() == [1, 1, 2] and counts[3:6].tolist() == [63, 64, 65]
    first_frame = np.concatenate([[0], np.cumsum(counts)])
    got, bad = _energy_twice(dev, signal, first_sample, n_samples, first_frame, win, hop)
    assert not bad.any()
    want = np.concatenate([V.energy_probs64(y, win, hop) for y in recs])
    host = np.concatenate([vad.EnergyScorer()(torch.from_numpy(np.lib.stride_tricks.sliding_window_view(y, win)[::hop].copy()), 16000).numpy()
                           for y in recs])
    # the NaN sample: exactly its own frames
    lo7 = int(first_frame[7])
    holds = np.array([t * hop <= nan_at < t * hop + win for t in range(counts[7])])
    assert holds.any() and not holds.all()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.flatnonzero(np.isnan(got)), lo7 + np.flatnonzero(holds))
    ok = ~np.isnan(want)
    d_dev, d_host = np.abs(got[ok].astype(np.float64) - want[ok]).max(), np.abs(host[ok].astype(np.float64) - want[ok]).max()
    bar = 16 * d_host + 2.0 ** -23
    print(f"(win, hop) = ({win}, {hop}): device against float64 {d_dev:.3e}, host EnergyScorer against float64 {d_host:.3e}, bar {bar:.3e}")
    assert bar < V.BAND, "the band of the end-to-end inputs must stay above the bar"
    assert d_dev <= bar
    lo8, lo9 = int(first_frame[8]), int(first_frame[9])
    assert np.all(got[lo8:lo9] < 1e-20) and np.all(got[lo8:lo9] > 0) and np.all(got[lo9:] > 0.999999)


def test_energy_flags(dev):
    """Every cause of `bad` of entry 1: a recording shorter than a frame, one that leaves the signal, one whose frame count disagrees"""
    win, hop = 480, 160
    rs = np.random.RandomState(9)
    recs = [(0.05 * rs.standard_normal(n)).astype(np.float32) for n in (win + 70 * hop, 300, win + 5 * hop + 7, win + 64 * hop)]
    signal, first_sample, n_samples = _pack(recs, [0, 1, 2, 3])
    counts = np.array([V.frame_count(n, win, hop) for n in n_samples])
    assert counts[1] == 0
    first_frame = np.concatenate([[0], np.cumsum(counts)])
    want = V.energy_entry(signal, first_sample, n_samples, first_frame, win, hop)
    assert want[1].tolist() == [0, V.SHORT, 0, 0]
    cases = [("short", first_sample, n_samples, first_frame, want)]
    ns = n_samples.copy()
    ns[3] += hop                                                               # one frame past the end of the signal
    ff = np.concatenate([[0], np.cumsum([V.frame_count(n, win, hop) for n in ns])])
    w = V.energy_entry(signal, first_sample, ns, ff, win, hop)
    assert w[1].tolist() == [0, V.SHORT, 0, V.BAD_RANGE] and np.isnan(w[0][ff[3]:]).all()
    cases.append(("range", first_sample, ns, ff, w))
    fs = first_sample.copy()
    fs[0] = -1
    w = V.energy_entry(signal, fs, n_samples, first_frame, win, hop)
    assert w[1].tolist() == [V.BAD_RANGE, V.SHORT, 0, 0]
    cases.append(("negative", fs, n_samples, first_frame, w))
    ff = first_frame.copy()
    ff[3:] -= 1                                                                # recording 2 is promised one frame fewer than it has
    w = V.energy_entry(signal, first_sample, n_samples, ff, win, hop)
    assert w[1].tolist() == [0, V.SHORT, V.BAD_FRAMES, 0]
    cases.append(("frames", first_sample, n_samples, ff, w))
    ff = first_frame.copy()
    ff[4] += 3                                                                 # the table ends past the frames of the last recording
    w = V.energy_entry(signal, first_sample, n_samples, ff, win, hop)
    assert w[1].tolist() == [0, V.SHORT, 0, V.BAD_FRAMES]
    cases.append(("end", first_sample, n_samples, ff, w))
    for name, fs_, ns_, ff_, (p64, bad64) in cases:
        got, bad = _energy_twice(dev, signal, fs_, ns_, ff_, win, hop)
        assert bad.tolist() == bad64.tolist(), name
        assert np.array_equal(np.isnan(got), np.isnan(p64)), name
        ok = ~np.isnan(p64)
        assert np.abs(got[ok] - p64[ok]).max() < 1e-5, name


# ------------------------------------------------------------------ the routes

def _signals():
    return [V.bursty_signal(sec, seed) for sec, seed in V.E2E_SIGNALS] + [V.silent_signal(2.0), np.zeros(4000, np.float32)]


def test_vad_segments_groups_equals_the_host_chain(dev):
    """The band-clean signals of tests/test_vad_rules.py: the region lists of `vad.silero_vad_segments`, exactly, in two launches"""
    from speech_diarization_amd import vad, vad_gpu
    ys = _signals()
    for kw in ({}, {"min_speech_ms": 350.0, "speech_pad_ms": 80.0, "morph_open_ms": 50.0}):
        want = [vad.silero_vad_segments(y, **kw) for y in ys]
        with expect_launches(exactly=KERNELS) as log:
            got = vad_gpu.vad_segments_groups(ys, **kw)
        assert log == {"vad_energy_kernel": 1, "vad_segments_kernel": 1}
        assert got == want and sum(len(w) for w in want) > 20 and want[-1] == [] and want[-2] == []
    with expect_launches(exactly=KERNELS):
        assert vad_gpu.vad_segments(ys[1]) == vad.silero_vad_segments(ys[1])
    # a real scorer's door: device probabilities in, regions and masks out
    p = torch.from_numpy(vad.using_silero_vad().probs(ys[2])).cuda()
    with expect_launches(exactly=SEGMENTS_KERNEL):
        segs, masks = vad_gpu.segments_from_probs_groups(p, [0, p.numel()], speech_pad_ms=40.0, return_mask=True)
    host_mask = vad.morph_open_close(vad.hysteresis_binarize(p.cpu().numpy(), 0.6, 0.4), 10.0)
    assert np.array_equal(masks[0], host_mask) and segs[0] == vad.mask_to_segments(host_mask, 10.0, speech_pad_ms=40.0)
    with expect_launches() as log:
        with pytest.raises(ValueError, match=r"Input is too short \(n=479\) for frame_length=480"):
            vad_gpu.vad_segments_groups([ys[0], ys[0][:479]])
        with pytest.raises(ValueError, match="segments_from_probs_groups"):
            vad_gpu.vad_segments_groups(ys[:1], scorer=lambda frames, sr: frames[:, 0])
    assert not KERNELS & set(log)


def test_the_diarizers_with_the_device_vad(dev, tmp_path):
    """Three short recordings, one of them without speech: segments, labels and RTTM bytes of vad="host", from `diarize_audios`,
    `diarize_audio` and `Diarizer`; the host's ValueError for a recording shorter than a frame"""
    from speech_diarization_amd import diarization_baseline as db, synth
    ys = [synth.synthetic_conversation(12.0, 2, seed=0).wav.astype(np.float32), np.zeros(3 * 16000, np.float32),
          synth.synthetic_conversation(8.0, 3, seed=1).wav.astype(np.float32)]
    audios = [{"waveform": y, "sample_rate": 16000, "uri": f"rec{i}"} for i, y in enumerate(ys)]
    paths = {route: [tmp_path / f"{route}{i}.rttm" for i in range(3)] for route in ("host", "device")}
    host = db.diarize_audios(audios, 0.35, 0.1, 2, 6, rttm_filepaths=paths["host"], return_details=True)
    with expect_launches(exactly=KERNELS) as log:
        device = db.diarize_audios(audios, 0.35, 0.1, 2, 6, rttm_filepaths=paths["device"], return_details=True, vad="device")
    assert log["vad_energy_kernel"] == 1 and log["vad_segments_kernel"] == 1
    for i, ((seg_h, det_h), (seg_d, det_d)) in enumerate(zip(host, device)):
        assert det_d["speech"] == det_h["speech"] and seg_d == seg_h and np.array_equal(det_d["labels"], det_h["labels"]), i
        assert paths["device"][i].read_bytes() == paths["host"][i].read_bytes(), i
    assert host[1][0] == [] and len(host[0][0]) and len(host[2][0])
    for i in (0, 1):
        one_h = db.diarize_audio(audios[i], 0.35, 0.1, 2, 6, clustering="ahc_gpu", return_details=True)
        with expect_launches(exactly=KERNELS):
            one_d = db.diarize_audio(audios[i], 0.35, 0.1, 2, 6, clustering="ahc_gpu", return_details=True, vad="device")
        assert one_d[0] == one_h[0] and one_d[1]["speech"] == one_h[1]["speech"] and np.array_equal(one_d[1]["labels"], one_h[1]["labels"])
    hp = db.DiarizationParameters()
    with expect_launches(exactly=KERNELS):
        assert db.Diarizer(hp, clustering="ahc_gpu", vad="device").diarize(audios[0], None) == db.Diarizer(hp, clustering="ahc_gpu").diarize(audios[0], None)
    short = {"waveform": ys[0][:400], "sample_rate": 16000, "uri": "short"}
    text = r"Input is too short \(n=400\) for frame_length=480"
    with expect_launches() as log:
        for route in ("host", "device"):
            with pytest.raises(ValueError, match=text):
                db.diarize_audios([audios[0], short], 0.35, 0.1, 2, 6, vad=route)
            with pytest.raises(ValueError, match=text):
                db.diarize_audio(short, 0.35, 0.1, 2, 6, clustering="ahc_gpu", vad=route)
            with pytest.raises(ValueError, match=text):
                db.Diarizer(hp, clustering="ahc_gpu", vad=route).diarize(short, None)
    assert not KERNELS & set(log)
