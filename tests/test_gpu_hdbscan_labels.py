"""HDBSCAN's labels on the GPU (include/sd_hip_tree.h, sd_tree_labels_grouped): exact integer equality of the label arrays with the
scikit-learn oracle of tests/helpers/hdbscan_labels_ref.py (`make_single_linkage` + `tree_to_labels` on the stably sorted edges), every
run held to its kernel by the launch log.  The oracle of a (tree, setting) is computed once per session and shared."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import guarded as G  # noqa: E402
import hdbscan_labels_ref as T  # noqa: E402
import hdbscan_ref as H  # noqa: E402
import launch_log as L  # noqa: E402

from speech_diarization_amd import _native as N  # noqa: E402
from speech_diarization_amd import cluster, hdbscan_gpu, ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNEL = "tree_labels_grouped_kernel"

_ORACLE = {}


def _oracle(name, tree, setting):
    if (name, setting) not in _ORACLE:
        _ORACLE[name, setting] = T.oracle_labels(*tree, *setting)
    return _ORACLE[name, setting]


def _run(trees, setting, max_edges=None):
    """One launch over the trees -> (one label array per recording, bad), under the launch log."""
    lo, hi, dist, first, most = T.pack(trees)
    up = [torch.from_numpy(a).to(DEV) for a in (lo, hi, dist, first)]
    with L.expect_launches(exactly={KERNEL}) as log:
        labels, bad = ops.tree_labels_grouped(*up, most if max_edges is None else max_edges, *setting)
        got = torch.cat([labels, bad]).cpu().numpy()
    assert log == {KERNEL: 1}, log
    n = len(dist) + len(trees)
    return T.unpack(got[:n], first), got[n:]


@pytest.fixture(scope="module")
def cases():
    return {name: (lo, hi, dist) for name, lo, hi, dist in T.random_cases()}


# ------------------------------------------------------------------ 1. the smallest shapes

@pytest.mark.parametrize("setting", T.SETTINGS)
def test_two_three_and_five_rows(setting):
    """n < min_cluster_size included; three rows without a single cluster is where a wrong root rule shows."""
    small = T.small_trees()
    assert {len(t[3]) + 1 for t in small} == {2, 3, 5}
    for name, *tree in small:
        (got,), bad = _run([tree], setting)
        assert bad.tolist() == [0] and got.dtype == np.int32 and np.array_equal(got, _oracle(name, tree, setting)), (name, got)
    together, bad = _run([t[1:] for t in small], setting)
    assert not bad.any() and all(np.array_equal(g, _oracle(t[0], t[1:], setting)) for g, t in zip(together, small))


# ------------------------------------------------------------------ 2. random trees

@pytest.mark.parametrize("n", T.SIZES)
def test_random_trees_equal_the_oracle(cases, n):
    """Three distance families (distinct; four values: heavy ties and the stable sort; a quarter at 0.0: lambda = inf and NaN
    stabilities) x three seeds, at the four settings; the nine trees of a size share a launch (test 3 holds a launch to its recordings
    alone)."""
    names = [f"{family}{n}s{seed}" for family in T.FAMILIES for seed in T.SEEDS]
    for setting in T.SETTINGS:
        got, bad = _run([cases[name] for name in names], setting)
        assert not bad.any(), bad
        for name, g in zip(names, got):
            want = _oracle(name, cases[name], setting)
            assert np.array_equal(g, want), (name, setting, int((g != want).sum()))


@pytest.mark.parametrize("n", [129, T.LDS_ROWS + 1])
def test_path_star_and_balanced_trees(cases, n):
    """The deepest dendrogram (a path), the one whose every edge ties (a star) and a shallow one with many true splits: the bounds on
    the union-find walks and on the two queues."""
    names = [f"path{n}", f"star{n}", f"balanced{n}"]
    for setting in T.SETTINGS:
        got, bad = _run([cases[name] for name in names], setting)
        assert not bad.any(), bad
        for name, g in zip(names, got):
            assert np.array_equal(g, _oracle(name, cases[name], setting)), (name, setting)


# ------------------------------------------------------------------ 3. many recordings in one launch

def test_forty_recordings_equal_their_own_launches_bitwise(cases):
    cap = T.LDS_ROWS
    sizes = [17, 64, 129, 500] * 8 + [cap, cap + 1, 2 * cap + 3, 17, cap + 1, 129, 64, cap]
    sizes = [sizes[(7 * i) % 40] for i in range(40)]                    # mixed: both sides of the cap stand between small ones
    assert len(sizes) == 40 and min(sizes) < cap < max(sizes)
    names = [f"{T.FAMILIES[i % 3]}{n}s{(i // 3) % 3}" for i, n in enumerate(sizes)]
    trees = [cases[name] for name in names]
    setting = (6, False)
    got, bad = _run(trees, setting)
    again, bad2 = _run(trees, setting)
    assert not bad.any() and not bad2.any()
    for name, tree, g, a in zip(names, trees, got, again):
        assert np.array_equal(g, a), name                               # run to run
        assert np.array_equal(g, _oracle(name, tree, setting)), name
    for name in sorted(set(names)):                                      # each alone
        (alone,), bad = _run([cases[name]], setting)
        assert bad.tolist() == [0] and np.array_equal(alone, got[names.index(name)]), name


# ------------------------------------------------------------------ 4. broken input

@pytest.mark.parametrize("kind", T.BREAKAGES)
def test_a_broken_recording_is_reported_and_the_others_are_not_touched(cases, kind):
    """Refusals by value: the entry compares every index with its range before it uses it (an index of n_g or -1 never becomes an
    address), a repeated edge shows as an edge inside one component in the union-find, and a NaN distance by its exponent bits.  All
    buffers stand between guard bands; the broken recording is once a small one (state in LDS) and once one above the cap (state in the
    guarded workspace)."""
    setting = (2, True)
    for names in (["distinct17s0", "four64s1", "zeros129s2"], ["four64s1", f"distinct{T.LDS_ROWS + 1}s0", "zeros17s2"]):
        trees = [cases[name] for name in names]
        trees[1] = T.break_tree(trees[1], kind)
        lo, hi, dist, first, most = T.pack(trees)
        E, n_groups = len(dist), 3
        need = int(N.load().sd_tree_labels_workspace_bytes(E, n_groups, most))
        assert (need == 0) == (most + 1 <= T.LDS_ROWS)
        bufs = {k: G.guarded_from(torch.from_numpy(v), DEV, name=k) for k, v in (("lo", lo), ("hi", hi), ("dist", dist), ("first_edge", first))}
        labels = G.guarded(4 * (E + n_groups), 0x7B, DEV, name="labels")
        bad = G.guarded(4 * n_groups, 0x7B, DEV, name="bad")
        ws = G.guarded(max(need, 16), 0xFF, DEV, name="ws")
        with L.expect_launches(exactly={KERNEL}):
            ops.launch("sd_tree_labels_grouped", labels.raw, bufs["lo"].ptr, bufs["hi"].ptr, bufs["dist"].ptr, bufs["first_edge"].ptr, n_groups, E,
                       most, setting[0], int(setting[1]), labels.ptr, bad.ptr, ws.ptr, max(need, 16))
            torch.cuda.synchronize()
        G.assert_guards_intact(labels, bad, ws, *bufs.values())
        for k, v in (("lo", lo), ("hi", hi), ("dist", dist), ("first_edge", first)):
            assert bytes(bufs[k].payload.cpu().numpy()) == v.tobytes(), k                              # the inputs are inputs
        per = T.unpack(labels.view(torch.int32).cpu().numpy(), first)
        verdict = bad.view(torch.int32).cpu().numpy()
        assert verdict[0] == 0 and verdict[1] != 0 and verdict[2] == 0, (kind, names, verdict)
        assert (per[1] == -1).all() and len(per[1]) == len(trees[1][2]) + 1
        for i in (0, 2):
            assert np.array_equal(per[i], _oracle(names[i], cases[names[i]], setting)), (kind, names[i])
    # more edges than the caller's bound is the same refusal
    trees = [cases[name] for name in ("distinct17s0", "four64s1", "zeros129s2")]
    got, bad = _run(trees, setting, max_edges=100)
    assert bad.tolist()[:2] == [0, 0] and bad[2] != 0 and (got[2] == -1).all() and np.array_equal(got[0], _oracle("distinct17s0", trees[0], setting))


# ------------------------------------------------------------------ 5. end to end

class Recording(hdbscan_gpu.DeviceRows):
    """The product operator; keeps what `tree_labels` was handed."""

    def tree_labels(self, lo, hi, dist, first_edge, *rest):
        self.seen = tuple(t.cpu().numpy() for t in (lo, hi, dist, first_edge))
        return super().tree_labels(lo, hi, dist, first_edge, *rest)


# the inputs of tests/test_hdbscan_labels_rules.py: seeds at which the weights of the tree are pairwise distinct at (2, None)
PLANTED = [(300, 4, 0.6, 0, 0), (500, 5, 0.8, 1, 10), (129, 3, 0.5, 5, 4)]
END_SETTINGS = [(2, None, True), (6, 3, False), (15, 5, True)]


@pytest.mark.parametrize("setting", END_SETTINGS)
def test_hdbscan_rows_and_groups_end_to_end(setting):
    mcs, ms, single = setting
    mats = [H.planted(*shape) for shape in PLANTED]
    per = []
    for x in mats:
        X = torch.from_numpy(x).to(DEV)
        op = Recording(X.device)
        with L.expect_launches(exactly={KERNEL}):
            got = hdbscan_gpu.hdbscan_rows(X, mcs, ms, single, operator=op, labelling="device")
        lo, hi, dist, first = op.seen
        assert first.tolist() == [0, len(x) - 1]
        assert np.array_equal(got, T.oracle_labels(lo, hi, dist, mcs, single)), (len(x), setting)
        if setting == (2, None, True):                                  # raw scores: no ties, so the scikit-learn route says the same
            assert len(np.unique(dist)) == len(dist), "the edge distances of this input tie: choose another seed"
            want = hdbscan_gpu.hdbscan_rows(X, mcs, ms, single, operator=op)
            assert got.dtype == want.dtype and np.array_equal(got, want), len(x)
        per.append(got)
    X = torch.from_numpy(np.concatenate(mats + [mats[0][:1]])).to(DEV)
    op = Recording(X.device)
    with L.expect_launches(exactly={KERNEL}) as log:
        many = hdbscan_gpu.hdbscan_rows_groups(X, [len(x) for x in mats] + [1], mcs, ms, single, operator=op, labelling="device")
    assert log[KERNEL] == 1 and many[3].tolist() == [0]
    lo, hi, dist, first = op.seen
    for g, (x, alone) in enumerate(zip(mats, per)):
        a, b = first[g], first[g + 1]
        assert np.array_equal(many[g], T.oracle_labels(lo[a:b], hi[a:b], dist[a:b], mcs, single)) and np.array_equal(many[g], alone), (g, setting)


def test_two_stage_device_factory_equals_the_sklearn_factory():
    x = H.planted(*PLANTED[2])                                          # several micro-clusters: stage 2 runs
    with L.expect_launches(exactly={KERNEL}) as log:
        got = cluster.cluster_hdbscan_two_stage(x, 2, clusterer_factory=hdbscan_gpu.HdbscanGpuClusterer.factory(labelling="device"))
    assert log[KERNEL] == 2                                             # both stages
    with L.launches() as log:
        want = cluster.cluster_hdbscan_two_stage(x, 2, clusterer_factory=hdbscan_gpu.HdbscanGpuClusterer.factory(labelling="sklearn"))
    assert KERNEL not in log
    assert got.dtype == want.dtype and np.array_equal(got, want) and len(set(got.tolist())) >= 2


def _fft_encoder(w):
    return np.stack([np.abs(np.fft.rfft(r, 382))[:192] for r in np.asarray(w, dtype=np.float32)]).astype(np.float32)


def _vad(y, sr, **kw):
    return [(0.5 * i, 0.5 * i + 0.45) for i in range(int(len(y) / sr / 0.5))]


def test_diarize_many_device_equals_diarize_device_per_recording():
    """Two short synthetic recordings, a stub encoder and a stub VAD; the clusterer is the product one on the GPU."""
    from speech_diarization_amd import anti_stick_diarize as asd
    from speech_diarization_amd import synth
    ys = [synth.synthetic_conversation(12.0, 2, seed=0).wav, synth.synthetic_conversation(8.0, 3, seed=1).wav]
    kw = dict(encode=_fft_encoder, vad_segments=_vad, scd_thr=1e9, reseg=0, clusterer="hdbscan_device")
    with L.expect_launches(exactly={KERNEL}) as log:
        want = [asd.diarize(y, **kw) for y in ys]
    assert log[KERNEL] >= 2
    with L.expect_launches(exactly={KERNEL}):
        got = asd.diarize_many(ys, **kw)
    triples = lambda segs: [(s.start, s.end, s.spk) for s in segs]  # noqa: E731
    assert [triples(g) for g in got] == [triples(w) for w in want] and all(len(g) >= 1 for g in got)
