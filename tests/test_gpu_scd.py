"""The device speaker-change detection on the MI355X (include/sd_hip_scd.h: sd_scd_split_grouped_f32; scd_gpu.py; scd="device" on
scd_split_segments, diarize and diarize_many): the entry against the numpy statement (tests/helpers/scd_ref.py) fed with the cosines of
`ops.adjacent_cosine` on each segment alone, which `sims` must equal bit for bit; counts, masks, flags and the bits of the piece
times; guard bands at exact buffer sizes; every cause of `bad` and every refusal; and the public routes against the host route.
Every launch runs under the launch log, held to its kernel, and twice with identical bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import guarded as G  # noqa: E402
import scd_ref as S  # noqa: E402
from launch_log import expect_launches  # noqa: E402

pytestmark = pytest.mark.gpu

KERNEL = {"scd_split_kernel"}
OUTPUTS = ("n_peaks", "n_pieces", "piece_start", "piece_end", "sims", "mask", "bad")


@pytest.fixture(scope="module")
def dev():
    from speech_diarization_amd import _native as N
    N.load()
    return torch.device("cuda")


def _fill(poison: int, dt):
    return np.frombuffer(bytes([poison] * 8), dt)[0]


def _bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def _tables(rows_list, first_row=None, first_piece=None):
    counts = np.array([len(r) for r in rows_list])
    fr = np.concatenate([[0], np.cumsum(counts)]) if first_row is None else np.asarray(first_row)
    fp = np.concatenate([[0], np.cumsum([S.capacity(n) for n in counts])]) if first_piece is None else np.asarray(first_piece)
    return counts, fr, fp


def _split(dev, rows_list, starts, ends, hop_ms, thr, min_speech_s, eps=1e-8, ld_extra=0, first_row=None, first_piece=None, want_sims=True,
           want_mask=True, poison=0xFF):
    """One call of the entry on guarded buffers of exactly the sizes the header names -> dict of numpy arrays.  `rows_list`: one f32
    [n, dim] per segment (n may be 0); the columns between dim and ld hold NaN; the tables default to the ones the driver would make."""
    from speech_diarization_amd import _native as N
    from speech_diarization_amd import ops
    counts, fr, fp = _tables(rows_list, first_row, first_piece)
    dim = rows_list[0].shape[1]
    ng, n_rows, cap, ld = len(rows_list), int(counts.sum()), int(fp[-1]), dim + ld_extra
    flat = np.full((n_rows, ld), np.nan, np.float32)
    flat[:, :dim] = np.concatenate(rows_list)
    flat = flat.reshape(-1)[:max(n_rows * ld - ld_extra, 0)]                                     # the last row ends at its dim: no tail
    rows = G.guarded_from(torch.from_numpy(flat.copy()), dev, "rows")
    t_fr = G.guarded_from(torch.from_numpy(fr.astype(np.int32)), dev, "first_row")
    t_fp = G.guarded_from(torch.from_numpy(fp.astype(np.int32)), dev, "first_piece")
    t_s = G.guarded_from(torch.from_numpy(np.asarray(starts, np.float64)), dev, "seg_start")
    t_e = G.guarded_from(torch.from_numpy(np.asarray(ends, np.float64)), dev, "seg_end")
    n_peaks, n_pieces, bad = (G.guarded(4 * ng, poison, dev, name) for name in ("n_peaks", "n_pieces", "bad"))
    piece_start, piece_end = (G.guarded(8 * cap, poison, dev, name) for name in ("piece_start", "piece_end"))
    sims, mask = G.guarded(4 * n_rows, poison, dev, "sims"), G.guarded(n_rows, poison, dev, "mask")
    need = int(N.load().sd_scd_split_workspace_bytes(n_rows, ng))
    assert need == 16 * n_rows
    ws = G.guarded(need, poison, dev, "ws")
    bufs = (rows, t_fr, t_fp, t_s, t_e, n_peaks, n_pieces, bad, piece_start, piece_end, sims, mask, ws)
    with expect_launches(exactly=KERNEL) as log:
        ops.launch("sd_scd_split_grouped_f32", ws.raw, rows.ptr, ld, dim, n_rows, t_fr.ptr, ng, t_s.ptr, t_e.ptr, C.c_double(hop_ms), C.c_double(thr),
                   C.c_double(min_speech_s), C.c_float(eps), t_fp.ptr, cap, n_peaks.ptr, n_pieces.ptr, piece_start.ptr, piece_end.ptr,
                   sims.ptr if want_sims else None, mask.ptr if want_mask else None, bad.ptr, ws.ptr, need)
        torch.cuda.synchronize()
    assert log == {"scd_split_kernel": 1}
    G.assert_guards_intact(*bufs)
    assert rows.view(torch.float32).cpu().numpy().tobytes() == flat.tobytes()                    # the inputs are only read
    out = {name: b.view(dt).cpu().numpy().copy() for name, b, dt in (
        ("n_peaks", n_peaks, torch.int32), ("n_pieces", n_pieces, torch.int32), ("piece_start", piece_start, torch.float64),
        ("piece_end", piece_end, torch.float64), ("sims", sims, torch.float32), ("mask", mask, torch.uint8), ("bad", bad, torch.int32))}
    return out


def _split_twice(dev, rows_list, starts, ends, hop_ms, thr, min_speech_s, **kw):
    """Two launches, a different poison under the outputs each time -> the results of the first, the slots the entry leaves alone
    holding that poison; what it writes is identical"""
    a = _split(dev, rows_list, starts, ends, hop_ms, thr, min_speech_s, poison=G.POISONS[0], **kw)
    b = _split(dev, rows_list, starts, ends, hop_ms, thr, min_speech_s, poison=G.POISONS[1], **kw)
    for name in OUTPUTS:
        x, y = _bits(a[name]), _bits(b[name])
        if name in ("piece_start", "piece_end"):
            wrote = (x != _bits(np.array([_fill(G.POISONS[0], np.float64)]))[0]) | (y != _bits(np.array([_fill(G.POISONS[1], np.float64)]))[0])
            assert np.array_equal(x[wrote], y[wrote]), name
        elif (name != "sims" or kw.get("want_sims", True)) and (name != "mask" or kw.get("want_mask", True)):
            assert np.array_equal(x, y), name
    return a


_COS = {}


def _device_cosines(dev, rows_list, eps=1e-8, key=None):
    """The cosines of `ops.adjacent_cosine` (the parent's kernel) on each segment ALONE, in the layout of `sims`"""
    from speech_diarization_amd import ops
    if key is not None and key in _COS:
        return _COS[key]
    parts = []
    for r in rows_list:
        if len(r) >= 2:
            parts.append(ops.adjacent_cosine(torch.from_numpy(np.ascontiguousarray(r)).to(dev), eps=eps).cpu().numpy())
        if len(r) >= 1:
            parts.append(np.array([np.nan], np.float32))
    cos = np.concatenate(parts) if parts else np.zeros(0, np.float32)
    if key is not None:
        _COS[key] = cos
    return cos


def _check(dev, rows_list, starts, ends, hop_ms, thr, min_speech_s, eps=1e-8, only=None, key=None, **kw):
    """Launch twice, state the same call from the device cosines, compare everything (segments `only`: a boolean vector, default all)
    -> (got, want)"""
    counts, fr, fp = _tables(rows_list, kw.get("first_row"), kw.get("first_piece"))
    got = _split_twice(dev, rows_list, starts, ends, hop_ms, thr, min_speech_s, eps=eps, **kw)
    cos = _device_cosines(dev, rows_list, eps, key)
    if kw.get("want_sims", True):
        ok = got["bad"][np.repeat(np.arange(len(counts)), counts)] == 0
        assert np.array_equal(_bits(got["sims"])[ok], _bits(cos)[ok]), "sims are not the bits of ops.adjacent_cosine"
        assert np.isnan(got["sims"][~ok]).all() and np.isnan(got["sims"][fr[1:][counts > 0] - 1]).all()
    want = S.split_entry(cos, fr, starts, ends, hop_ms, thr, min_speech_s, fp, piece_fill=_fill(G.POISONS[0], np.float64))
    only = np.ones(len(counts), bool) if only is None else only
    assert np.array_equal(got["bad"], want["bad"])
    for name in ("n_peaks", "n_pieces"):
        assert np.array_equal(got[name][only], want[name][only]), (name, np.flatnonzero(got[name] != want[name])[:5])
    for g in np.flatnonzero(only):
        a, b, q = int(fr[g]), int(fr[g + 1]), slice(int(fp[g]), int(fp[g + 1]))
        if kw.get("want_mask", True):
            assert np.array_equal(got["mask"][a:b], want["mask"][a:b]), g
        for name in ("piece_start", "piece_end"):
            assert np.array_equal(_bits(got[name][q]), _bits(want[name][q])), (name, g, got[name][q], want[name][q])
    return got, want


def _times(n):
    return np.arange(n) * 50.0 + 0.25


# ------------------------------------------------------------------ the smallest shapes

@pytest.mark.parametrize("dim,ld_extra", [(192, 0), (5, 3)])
def test_short_segments_and_the_smallest_peak(dev, dim, ld_extra):
    """Segments of 0, 1, 2, 3, 4 and 5 rows in one launch: fewer than 3 rows pass through whatever min_speech_s is, 3 rows can have no
    peak, 4 rows have their only candidate at index 1"""
    rs = np.random.RandomState(dim)
    rows = [np.zeros((0, dim), np.float32), S.rows_with_cosines([], dim, rs), S.rows_with_cosines([0.3], dim, rs), S.rows_with_cosines([0.9, 0.2], dim, rs),
            S.rows_with_cosines([0.9, 0.2, 0.9], dim, rs), S.rows_with_cosines([0.9, 0.3, 0.95, 0.5], dim, rs), np.zeros((0, dim), np.float32),
            S.rows_with_cosines([0.2, 0.9, 0.9], dim, rs)]
    starts = _times(len(rows))
    ends = starts + np.array([0.5, 1.0, 1.2, 1.4, 1.6, 1.8, 0.0, 1.6])
    for thr, ms in ((1.0, 0.1), (1.0, 5.0), (-1e9, 0.0), (1e9, 0.1), (np.inf, 0.1)):
        got, want = _check(dev, rows, starts, ends, 200.0, thr, ms, ld_extra=ld_extra)
        assert got["n_peaks"][:4].tolist() == [0, 0, 0, 0] and got["n_pieces"][:4].tolist() == [1, 1, 1, 1] and got["n_peaks"][6:].tolist() == [0, 0]
        assert np.array_equal(got["piece_start"][:4], starts[:4]) and np.array_equal(got["piece_end"][:4], ends[:4])
        if thr <= 1.0:
            assert got["n_peaks"][4] == 1 and got["mask"][3 + 3 + 1] == 1 and got["mask"].sum() == got["n_peaks"].sum() == 2
            assert got["n_pieces"][4] == (2 if ms <= 0.1 else 0)
        else:
            assert not got["n_peaks"].any() and not got["mask"].any() and (got["n_pieces"] == 1).all()
    got, _ = _check(dev, rows, starts, ends, 200.0, 1.0, 0.1, ld_extra=ld_extra, want_sims=False, want_mask=False)
    assert np.all(_bits(got["sims"]) == 0xFFFFFFFF) and np.all(got["mask"] == G.POISONS[0])          # null outputs: nothing written


def test_sims_are_the_bits_of_adjacent_cosine_for_every_eps(dev):
    """`sims` against `ops.adjacent_cosine` on each segment alone, bit for bit (`_check` compares them), the last slot of every segment
    NaN, for three values of eps, rows of very different lengths, and a padded row stride"""
    rs = np.random.RandomState(1)
    rows = [(S.rows_with_cosines(S.cosine_family("uniform", n - 1, rs), 192, rs) * 10.0 ** rs.uniform(-3, 3)).astype(np.float32) for n in (2, 3, 9, 70, 1, 300)]
    starts = _times(len(rows))
    for eps, ld_extra in ((1e-8, 0), (0.0, 1), (0.5, 4)):
        got, _ = _check(dev, rows, starts, starts + 20.0, 200.0, 1.25, 1.0, eps=eps, ld_extra=ld_extra)
        assert np.isnan(got["sims"]).sum() == len(rows) and got["n_peaks"].sum() > 10


# ------------------------------------------------------------------ exact plateaus

def _word_rows(word, dim=24, seed=3):
    return S.codebook_rows(word, dim, seed)


def test_exact_plateaus(dev):
    """Rows from a codebook: the cosine of (A, B) has the bits of (B, A), so A A B A A gives d = [0, x, x, 0] and the peak is index 1;
    a plateau of three; a plateau touching index m - 1 is no peak, nor is one touching index 0; a peak at index 1 and one at m - 2"""
    words = ["AABAA", "AABABB", "AABA", "ABAA", "AABBBBAA", "AABABAA", "AAAA", "ABABAB"]
    rows = [_word_rows(w) for w in words]
    starts = _times(len(rows))
    got, want = _check(dev, rows, starts, starts + 30.0, 200.0, 0.5, 0.0)
    fr = np.concatenate([[0], np.cumsum([len(w) for w in words])])
    peaks = [np.flatnonzero(got["mask"][a:b]).tolist() for a, b in zip(fr[:-1], fr[1:])]
    assert peaks == [[1], [2], [], [], [1, 5], [2], [], []], peaks
    sims = got["sims"]
    assert sims[fr[0] + 1] == sims[fr[0] + 2] and sims[fr[1] + 1] == sims[fr[1] + 2] == sims[fr[1] + 3] and sims[fr[0] + 1] < 0.9
    assert got["n_pieces"].tolist() == [2, 2, 1, 1, 3, 2, 1, 1]


def test_the_branch_of_a_tiny_std(dev):
    """Near-identical rows: the distances are a few ulps of 1 and std <= 1e-6, so z = d: thr = 0.0 keeps the peaks, thr = 1e-3 none"""
    rs = np.random.RandomState(5)
    a = rs.standard_normal(64)
    e = rs.standard_normal(64)
    e -= e.dot(a) / a.dot(a) * a
    b = a + 1e-3 * np.linalg.norm(a) * e / np.linalg.norm(e)
    rows = [np.stack([a, a, b, b, a, a]).astype(np.float32), np.stack([a] * 5).astype(np.float32)]
    starts = _times(2)
    got, want = _check(dev, rows, starts, starts + 10.0, 200.0, 0.0, 0.0)
    d = 1.0 - got["sims"][:5].astype(np.float64)
    assert d.std() < 1e-6 and d.max() < 2e-6 and np.flatnonzero(got["mask"]).tolist() == [1, 3] and got["n_peaks"].tolist() == [2, 0]
    got, _ = _check(dev, rows, starts, starts + 10.0, 200.0, 1e-3, 0.0)
    assert not got["n_peaks"].any() and not got["mask"].any() and got["n_pieces"].tolist() == [1, 1]


def test_a_nan_row_takes_the_branch_z_equals_d_and_touches_no_other_segment(dev):
    rs = np.random.RandomState(6)
    rows = [S.rows_with_cosines(S.cosine_family("drops", n - 1, rs), 16, rs) for n in (20, 30, 25)]
    starts = _times(3)
    clean, _ = _check(dev, rows, starts, starts + 8.0, 200.0, 0.3, 0.4)
    assert clean["n_peaks"].all()
    dirty = [r.copy() for r in rows]
    dirty[1][11, 3] = np.nan
    got, want = _check(dev, dirty, starts, starts + 8.0, 200.0, 0.3, 0.4)
    assert np.isnan(got["sims"][20 + 10]) and np.isnan(got["sims"][20 + 11]) and np.isnan(got["sims"]).sum() == 3 + 2
    # z = d: the peaks are those whose distance itself reaches thr, and none next to the NaN
    d = 1.0 - got["sims"][20:49]
    assert np.flatnonzero(got["mask"][20:50]).tolist() == [p for p in S.peaks_of(d) if d[p] >= 0.3] and got["n_peaks"][1] > 0
    for g, (a, b) in enumerate(((0, 20), (50, 75))):
        g = 2 * g
        assert np.array_equal(got["mask"][a:b], clean["mask"][a:b]) and got["n_pieces"][g] == clean["n_pieces"][g]
    q = [0, 10, 25, 37]
    for g in (0, 2):
        assert np.array_equal(_bits(got["piece_start"][q[g]:q[g + 1]]), _bits(clean["piece_start"][q[g]:q[g + 1]]))


# ------------------------------------------------------------------ the greedy filter

def _rows_with_peaks(n, peaks, dim=24, seed=7):
    """n rows over a codebook of two vectors: the letter changes at the pairs `peaks`, so d is one high value there and ~0 elsewhere"""
    word, letter = "A", 0
    for i in range(n - 1):
        letter ^= i in peaks
        word += "AB"[letter]
    return S.codebook_rows(word, dim, seed)


def test_the_greedy_filter_on_hand_made_times(dev):
    """Cuts closer than min_speech_s are skipped, a tail shorter than min_speech_s is dropped, a segment emits no piece at all, and
    min_speech_s = 0 with peaks that round to the same cut: the times are compared as bits against the statement"""
    rows = [_rows_with_peaks(20, (2, 4, 12)), _rows_with_peaks(5, (1,)), _rows_with_peaks(30, (1, 3, 5, 7, 9, 11, 20, 27)),
            _rows_with_peaks(12, (3, 8))]
    starts = np.array([10.0, 100.3, 0.1 + 0.2, 7.7])
    ends = starts + np.array([3.0, 0.8, 6.05, 3.0])
    got, want = _check(dev, rows, starts, ends, 200.0, 0.5, 1.0)
    assert got["n_peaks"].tolist() == [3, 1, 8, 2] and got["n_pieces"].tolist() == [1, 0, 4, 2]
    assert got["piece_start"][0] == 10.0 and got["piece_end"][0] == 10.0 + 12.5 * 200.0 / 1000.0
    q2 = 10 + 2
    assert np.array_equal(got["piece_end"][q2:q2 + 4], [starts[2] + (p + 0.5) * 200.0 / 1000.0 for p in (5, 11, 20, 27)])
    # min_speech_s = 0 and a hop so small that every cut rounds to seg_start: one cut is left of the three
    rows = [_rows_with_peaks(12, (2, 5, 8)), _rows_with_peaks(12, (2, 5, 8))]
    starts, ends = np.array([1000.0, 0.0]), np.array([1002.0, 2.0])
    got, want = _check(dev, rows, starts, ends, 1e-13, 0.5, 0.0)
    assert got["n_peaks"].tolist() == [3, 3] and got["n_pieces"].tolist() == [2, 4]
    assert got["piece_start"][:2].tolist() == [1000.0, 1000.0] and got["piece_end"][:2].tolist() == [1000.0, 1002.0]
    got, want = _check(dev, rows, starts, ends, 200.0, 0.5, -1.0)                # a negative min_speech_s accepts every cut
    assert got["n_pieces"].tolist() == [4, 4]


# ------------------------------------------------------------------ random launches

@pytest.mark.parametrize("which", ("folder", "long"))
def test_random_launches_equal_the_statement(dev, which):
    """200 segments of 3-40 rows (dim 16), the four families driven through row constructions; and one segment of
    SD_SCD_LDS_ROWS + 1 rows (dim 8), whose lists live in the workspace.  Counts, masks and the bits of the piece times for every
    segment whose value margin is at least 1e-4; at most 1 % may lie below (tests/test_scd_rules.py holds the seed to that)"""
    rows, fr, starts, ends = S.random_launch() if which == "folder" else S.long_segment()
    assert which == "folder" or len(rows[0]) == S.LDS_ROWS + 1
    below = split = total = 0
    for thr in S.THRS:
        cos = _device_cosines(dev, rows, key=which)
        ref = S.split_entry(cos, fr, starts, ends, 200.0, thr, 1.0, _tables(rows)[2])
        only = ref["value_margin"] >= S.MARGIN
        got, want = _check(dev, rows, starts, ends, 200.0, thr, 1.0, only=only, key=which)
        below, split, total = below + int((~only).sum()), split + int((got["n_peaks"] > 0).sum()), total + len(rows)
    print(f"{which}: {total} segments, {below} below the margin, {split} split")
    assert below <= 0.01 * total and split >= (400 if which == "folder" else 4)


# ------------------------------------------------------------------ flags and refusals

def test_every_cause_of_bad(dev):
    rs = np.random.RandomState(8)
    rows = [S.rows_with_cosines(S.cosine_family("drops", n - 1, rs), 16, rs) for n in (12, 30, 2, 9)]
    starts = _times(4)
    ends = starts + 7.0
    counts, fr, fp = _tables(rows)
    # a share one piece too small: that segment alone (the next one gets the slot, so the table keeps its promise)
    small = fp.copy()
    small[2] -= 1
    got, want = _check(dev, rows, starts, ends, 200.0, 0.5, 0.3, first_piece=small)
    assert got["bad"].tolist() == [0, S.BAD_CAPACITY, 0, 0] and got["n_pieces"][1] == 0 and got["n_peaks"][1] == 0 and not got["mask"][12:42].any()
    assert np.isnan(got["sims"][12:42]).all() and got["n_peaks"][0] and got["n_peaks"][3]
    # a broken promise, in either table, at either end or in the middle: every segment, nothing written but NaN and zeros
    for name, table, broken in (("first_row", fr, [(0, 1), (2, int(fr[1]) - 1), (4, int(fr[4]) - 1), (3, int(fr[4]) + 1), (1, -1)]),
                                ("first_piece", fp, [(0, 1), (2, int(fp[1]) - 1), (3, int(fp[4]) + 1), (1, -5)])):
        for at, value in broken:
            t = table.copy()
            t[at] = value
            got = _split_twice(dev, rows, starts, ends, 200.0, 0.5, 0.3, **{name: t})
            assert got["bad"].tolist() == [S.BAD_PROMISE] * 4 and not got["n_peaks"].any() and not got["n_pieces"].any(), (name, at, value)
            assert not got["mask"].any() and np.isnan(got["sims"]).all()
            assert np.all(_bits(got["piece_start"]) == _bits(np.array([_fill(G.POISONS[0], np.float64)]))[0])


def test_every_refusal_comes_before_any_launch(dev):
    """Every SD_ERR_* of the header through the entry on real buffers: the status, and no launch in the log"""
    from speech_diarization_amd import _native as N
    lib = N.load()
    rows = torch.zeros((40, 8), dtype=torch.float32, device=dev)
    ints = torch.zeros((64,), dtype=torch.int32, device=dev)                 # five tables of eight, each its own
    first_row, first_piece, n_peaks, n_pieces, bad = (ints.data_ptr() + 32 * k for k in range(5))
    dbl = torch.zeros((64,), dtype=torch.float64, device=dev)
    ws = torch.zeros((1024,), dtype=torch.uint8, device=dev)
    good = dict(rows=rows.data_ptr(), ld=8, dim=8, n_rows=40, first_row=first_row, n_segs=4, seg_start=dbl.data_ptr(), seg_end=dbl.data_ptr() + 64,
                hop_ms=200.0, thr=1.25, min_speech_s=1.0, eps=1e-8, first_piece=first_piece, piece_cap=20, n_peaks=n_peaks,
                n_pieces=n_pieces, piece_start=dbl.data_ptr() + 128, piece_end=dbl.data_ptr() + 320, sims=None, peak_mask=None, bad=bad,
                ws=ws.data_ptr(), ws_bytes=640)
    cases = [(dict(n_segs=0), -1), (dict(n_segs=-1), -1), (dict(n_rows=-1), -1), (dict(piece_cap=-1), -1), (dict(dim=0), -1), (dict(ld=7), -1),
             (dict(hop_ms=float("nan")), -1), (dict(hop_ms=float("inf")), -1), (dict(min_speech_s=float("inf")), -1), (dict(min_speech_s=float("nan")), -1),
             (dict(eps=float("inf")), -1), (dict(eps=float("nan")), -1), (dict(thr=float("nan")), -1), (dict(ws=ws.data_ptr() + 4), -1),
             (dict(ws_bytes=639), -3), (dict(ws_bytes=0), -3)]
    cases += [({name: None}, -1) for name in ("rows", "first_row", "seg_start", "seg_end", "first_piece", "n_peaks", "n_pieces", "piece_start",
                                              "piece_end", "bad", "ws")]
    with expect_launches() as log:
        for change, code in cases:
            a = dict(good, **change)
            status = lib.sd_scd_split_grouped_f32(*a.values(), None)
            assert status == code and N.last_error().startswith("sd_scd_split_grouped_f32: "), (change, status, N.last_error())
        torch.cuda.synchronize()
    assert not KERNEL & set(log)
    with expect_launches(exactly=KERNEL):                # and the same buffers are accepted: first_row all 0 with n_rows 40 breaks the promise
        assert lib.sd_scd_split_grouped_f32(*good.values(), None) == 0
        torch.cuda.synchronize()
    assert ints[32:36].tolist() == [S.BAD_PROMISE] * 4 and not ints[:32].any()


# ------------------------------------------------------------------ the routes

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


def _conversations():
    from speech_diarization_amd import synth
    return [synth.synthetic_conversation(20.0, 2, seed=0).wav.astype(np.float32), synth.synthetic_conversation(12.0, 3, seed=1).wav.astype(np.float32)]


def test_scd_split_segments_on_the_device_equals_the_host_route(dev, small_encoder):
    """synthetic_conversation(20 s, 2 voices, seed 0) and (12 s, 3 voices, seed 1), each as one segment and as two halves, at thr 1.0
    and 1.5: scd="device" equals scd="host" piece for piece, unsplit segments as the same objects.  The value margins the statement
    reports for these segments from the device's cosines (printed, and asserted to be at least 1e-4), measured on the MI355X: 0.036,
    0.039, 0.039 for the three segments of the first recording and 0.036, 0.044, 0.035 for those of the second, at either threshold:
    with this encoder the closest decision of every segment is std > 1e-6 (the std of its distances is about 0.04), and no z lies
    that close to a threshold."""
    from speech_diarization_amd import anti_stick_diarize as asd
    margins = []
    for y in _conversations():
        total = len(y) / 16000
        segs = [asd.Segment(0.3, total - 0.1), asd.Segment(0.0, total / 2), asd.Segment(total / 2 + 0.2, total), asd.Segment(1.0, 1.9)]
        for thr in (1.0, 1.5):
            host = asd.scd_split_segments(y, 16000, segs, thr=thr)
            with expect_launches(exactly=KERNEL) as log:
                device = asd.scd_split_segments(y, 16000, segs, thr=thr, scd="device")
            assert log["scd_split_kernel"] == 1
            for seg in segs[:3]:
                a = int(seg.start * 16000)
                n = 1 + (len(y[a:int(seg.end * 16000)]) - 16000) // 3200
                rows = small_encoder.encode_windows(y, a + 3200 * np.arange(n), 16000, to_host=False)
                from speech_diarization_amd import ops
                margins.append(S.split_from_cosines(ops.adjacent_cosine(rows).cpu().numpy(), seg.start, seg.end, 200.0, thr, 1.0)[3])
            assert [(s.start, s.end) for s in device] == [(s.start, s.end) for s in host] and len(host) >= len(segs)
            assert [d is h for d, h in zip(device, host)] == [any(h is s for s in segs) for h in host] and device[-1] is segs[3]
    print("value margins:", " ".join(f"{m:.3g}" for m in margins))
    assert min(margins) >= S.MARGIN


def test_diarize_many_with_the_device_scd_equals_diarize_per_recording(dev, small_encoder):
    """Two conversations, a silent recording and one with a single short segment: `diarize_many(scd="device")` gives each what
    `diarize(scd="device", clusterer="hdbscan_gpu")` gives it alone (the same window launches, the same rows: no margin is needed),
    with ONE split launch for the folder"""
    from speech_diarization_amd import anti_stick_diarize as asd
    ys = _conversations()
    ys = [ys[0], np.zeros(3 * 16000, np.float32), ys[1], ys[0][:int(0.9 * 16000)]]
    kw = dict(scd_thr=1.0, scd="device")
    with expect_launches(exactly=KERNEL) as log:
        want = [asd.diarize(y, clusterer="hdbscan_gpu", **kw) for y in ys]
    per_recording = log["scd_split_kernel"]
    with expect_launches(exactly=KERNEL) as log:
        got = asd.diarize_many(ys, **kw)
    assert log["scd_split_kernel"] == 1 and per_recording >= 2
    assert [[(s.start, s.end, s.spk) for s in g] for g in got] == [[(s.start, s.end, s.spk) for s in w] for w in want]
    assert got[1] == [] and len(got[0]) >= 1 and len(got[2]) >= 1
