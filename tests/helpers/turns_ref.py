"""The numpy statement of sd_turns_grouped (include/sd_hip_turns.h): the rules of the header, one recording at a time, in the per-window
form the kernel uses (every window finds the first frame it owns by a binary search on the f64 comparison of rule 2), with the flags,
the slots that stay untouched, and a `numpy_launch` of the signature of `turns_gpu.turns_launch` for the CPU tests of the driver.
tests/test_turns_rules.py holds it equal to `cluster.relabel_by_first_appearance` + `diarization_baseline.labels_to_turns`."""
import numpy as np

BAD_LABEL, BAD_PROMISE = 1, 2
LDS_WINDOWS = 4096
MARGIN = 2.0 ** -40


def relabel(labels):
    """Rule 1: labels >= 0 numbered by first appearance, negative ones -1"""
    labels = np.asarray(labels, dtype=np.int64)
    out = np.full(labels.shape, -1, dtype=np.int64)
    keep = np.flatnonzero(labels >= 0)
    if keep.size:
        values, first = np.unique(labels[keep], return_index=True)
        number = np.empty(len(values), dtype=np.int64)
        number[np.argsort(first, kind="stable")] = np.arange(len(values))
        out[keep] = number[np.searchsorted(values, labels[keep])]
    return out


def frame_time(start, i, frame_s):
    """Rule 2: region_start + (i + 0.5) * frame_s in f64, in this order"""
    return start + (np.asarray(i, dtype=np.int64) + 0.5) * frame_s


def region_of(rfw, n):
    """The region of each of the n windows of a recording: the last q with rfw[q] <= w (rfw: nr + 1 entries from 0 to n)"""
    return np.searchsorted(rfw, np.arange(n), side="right") - 1


def promise_of_a_recording(rfw, centre, region_start, n_frames, frame_s):
    """Rule 4 for one recording (rfw counted from its first window): the slice of region_first_window, the frame counts, and per window
    the finite extent E of its region and the margin E * 2^-40 between neighbouring centres"""
    n, nr = len(centre), len(region_start)
    rfw = np.asarray(rfw, dtype=np.int64)
    if len(rfw) != nr + 1 or rfw[0] != 0 or rfw[-1] != n or np.any(np.diff(rfw) < 0) or np.any(np.asarray(n_frames) < 1):
        return False
    if n == 0:
        return True
    reg = region_of(rfw, n)
    a, b = rfw[reg], rfw[reg + 1] - 1
    s, nf = np.asarray(region_start, np.float64)[reg], np.asarray(n_frames, np.int64)[reg]
    with np.errstate(invalid="ignore", over="ignore"):
        t_0, t_last = frame_time(s, 0, frame_s), frame_time(s, nf - 1, frame_s)
        d = np.abs(np.stack([t_0 - centre[a], t_0 - centre[b], t_last - centre[a], t_last - centre[b]]))
        finite = np.all(d <= np.finfo(np.float64).max, axis=0)
        E = d.max(axis=0)
        gap = centre - np.roll(centre, 1)
        ok = finite & ((np.arange(n) == a) | (gap >= E * MARGIN))
    return bool(np.all(ok))


def first_frames(rfw, centre, region_start, n_frames, frame_s):
    """f_j of every window: 0 for the first window of a region, otherwise the first frame that is nearer to window j than to window
    j - 1 (n_frames when there is none), by the kernel's binary search -> (f, region of the window)"""
    n = len(centre)
    reg = region_of(rfw, n)
    s, nf = np.asarray(region_start, np.float64)[reg], np.asarray(n_frames, np.int64)[reg]
    before = np.roll(centre, 1)
    lo, hi = np.zeros(n, np.int64), np.where(np.arange(n) == np.asarray(rfw)[reg], 0, nf)
    while True:
        active = lo < hi
        if not active.any():
            return lo, reg
        mid = lo + ((hi - lo) >> 1)
        t = frame_time(s, mid, frame_s)
        nearer = np.abs(t - centre) < np.abs(t - before)
        hi = np.where(active & nearer, mid, hi)
        lo = np.where(active & ~nearer, mid + 1, lo)


def runs_of_a_recording(rfw, centre, region_start, n_frames, frame_s, new_labels):
    """Rules 2 and 3 for one recording that keeps its promises -> (run_region, run_first, run_end, run_label), int64 arrays"""
    n = len(centre)
    empty = np.zeros(0, np.int64)
    if n == 0:
        return empty, empty, empty, empty
    centre, new_labels = np.asarray(centre, np.float64), np.asarray(new_labels, np.int64)
    f, reg = first_frames(rfw, centre, region_start, n_frames, frame_s)
    nf = np.asarray(n_frames, np.int64)[reg]
    same_next = np.append(reg[1:] == reg[:-1], False)
    owners = np.flatnonzero(f < np.where(same_next, np.roll(f, -1), nf))
    head = np.ones(len(owners), bool)
    head[1:] = (reg[owners[1:]] != reg[owners[:-1]]) | (new_labels[owners[1:]] != new_labels[owners[:-1]])
    h = owners[head]
    run_region, run_first = reg[h], f[h]
    continues = np.append(run_region[1:] == run_region[:-1], False)
    run_end = np.where(continues, np.roll(run_first, -1), nf[h])
    return run_region, run_first, run_end, new_labels[h]


def tables_hold(first_window, first_region, n_windows, n_regions):
    """The promise about first_window and first_region, whose breach flags every recording"""
    for t, last in ((np.asarray(first_window, np.int64), n_windows), (np.asarray(first_region, np.int64), n_regions)):
        if t[0] != 0 or t[-1] != last or np.any(np.diff(t) < 0) or t.min() < 0 or t.max() > last:
            return False
    return True


def turns_entry(first_window, first_region, region_first_window, centre, region_start, n_frames, frame_s, labels, fill=-7):
    """The entry: dict of new_labels, run_region, run_first, run_end, run_label (int32 [W], untouched slots holding `fill`), n_runs and
    bad (int32 [G])"""
    G, W, R = len(first_window) - 1, len(labels), len(region_first_window) - 1
    out = {name: np.full(W, fill, np.int32) for name in ("new_labels", "run_region", "run_first", "run_end", "run_label")}
    out["n_runs"], out["bad"] = np.zeros(G, np.int32), np.zeros(G, np.int32)
    if not tables_hold(first_window, first_region, W, R):
        out["bad"][:] = BAD_PROMISE
        return out
    centre, labels = np.asarray(centre, np.float64), np.asarray(labels, np.int64)
    for g in range(G):
        a, b, r0, r1 = int(first_window[g]), int(first_window[g + 1]), int(first_region[g]), int(first_region[g + 1])
        rfw = np.asarray(region_first_window[r0:r1 + 1], np.int64) - a
        flag = BAD_LABEL if np.any(labels[a:b] >= b - a) else 0
        if not promise_of_a_recording(rfw, centre[a:b], region_start[r0:r1], n_frames[r0:r1], frame_s):
            flag |= BAD_PROMISE
        out["bad"][g] = flag
        if flag:
            continue
        new = relabel(labels[a:b])
        out["new_labels"][a:b] = new
        runs = runs_of_a_recording(rfw, centre[a:b], region_start[r0:r1], n_frames[r0:r1], frame_s, new)
        k = len(runs[0])
        out["n_runs"][g] = k
        for name, values in zip(("run_region", "run_first", "run_end", "run_label"), runs):
            out[name][a:a + k] = values
    return out


def numpy_launch(first_window, first_region, region_first_window, centre, region_start, n_frames, frame_s, labels):
    """`turns_gpu.turns_launch` on the host, for the tests of the driver"""
    o = turns_entry(first_window, first_region, region_first_window, centre, region_start, n_frames, frame_s, labels)
    return o["new_labels"], o["n_runs"], o["run_region"], o["run_first"], o["run_end"], o["run_label"], o["bad"]


# ------------------------------------------------------------------ cases

def tables_of(recordings):
    """[(rfw counted from the recording's first window, centre, region_start, n_frames, labels)] -> the seven tables of a launch"""
    fw, fr, rfw_all, centre, start, frames, labels = [0], [0], [], [], [], [], []
    for rfw, c, s, nf, lab in recordings:
        rfw_all.append(np.asarray(rfw[:-1], np.int64) + fw[-1])
        fw.append(fw[-1] + len(c)), fr.append(fr[-1] + len(s))
        centre.append(np.asarray(c, np.float64)), start.append(np.asarray(s, np.float64))
        frames.append(np.asarray(nf, np.int64)), labels.append(np.asarray(lab, np.int64))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)      # noqa: E731
    return (np.array(fw, np.int64), np.array(fr, np.int64), np.append(cat(rfw_all, np.int64), fw[-1]), cat(centre, np.float64),
            cat(start, np.float64), cat(frames, np.int64), cat(labels, np.int64))


def even_recording(counts, labels, hop=0.25, frame_s=0.01, start=0.0, gap=1.0):
    """A recording whose region q has counts[q] windows `hop` apart (a region may have none) and as many frames as cover them"""
    rfw, centre, starts, frames, t = [0], [], [], [], start
    for n in counts:
        length = max(n, 1) * hop
        centre += [t + hop * (j + 0.5) for j in range(n)]
        starts.append(t), frames.append(max(1, int(round(length / frame_s)))), rfw.append(rfw[-1] + n)
        t += length + gap
    labels = np.asarray(labels, np.int64)
    assert len(labels) == rfw[-1]
    return np.array(rfw), np.array(centre, np.float64), np.array(starts, np.float64), np.array(frames, np.int64), labels


def random_folder(seed=0, n_recordings=40):
    """About 40 recordings of 0-600 windows in regions of 0-40 windows, labels of 1-6 speakers with -1 mixed in; recording 17 has no
    windows (and two regions), and some regions of the others have none"""
    rs = np.random.RandomState(seed)
    recs = []
    for g in range(n_recordings):
        counts = [] if g == 5 else [int(c) for c in rs.randint(0, 41, rs.randint(1, 16))]
        if g == 17:
            counts = [0, 0]
        elif counts and g % 3 == 0:
            counts[len(counts) // 2] = 0
        n = sum(counts)
        k = rs.randint(1, 7)
        labels = np.repeat(rs.randint(-1, k, n // 3 + 1), 3)[:n] if g % 2 else rs.randint(-1, k, n)
        recs.append(even_recording(counts, np.minimum(labels, n - 1), hop=0.25 + 0.01 * g, start=0.0123 * g))
    return recs
