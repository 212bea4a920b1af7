"""Device route for the reference's density clustering: HDBSCAN from the rows themselves, without the N x N matrix.

`anti_stick_diarize.diarize()` clusters with `cluster_hdbscan_two_stage(embs, min_cluster_size=2)` [REF anti_stick_diarize.py:536], and
`cluster_hdbscan` / `diar_diag.cluster_embeddings(method="hdbscan")` are HDBSCAN as well; all go through
`cluster.default_hdbscan_factory` (scikit-learn's `HDBSCAN`), which forms the f64 N x N distance matrix on the host.  HDBSCAN's only
O(N^2) work is two steps, and on unit rows both are statements about cosines (a distance falls as the cosine grows):

    core[i]  = the (min_samples - 1)-th largest <x_i, x_j> over j != i          (scikit-learn counts the point itself)
    w(i, j)  = min(core[i], core[j], <x_i, x_j>)                                (mutual reachability, in cosine space)

and the minimum spanning tree of the mutual-reachability DISTANCE is the MAXIMUM spanning tree of w.  Everything after the tree is
O(N log N) on N - 1 edges and stays on the host with scikit-learn's own routines.

The steps
1. unit rows (`ops.l2norm_rows(..., sklearn_zero_guard=True)`), columns padded to a multiple of 4;
2. the core values, once (`ops.hdb_core`, `sd_hdb_core_f32`, include/sd_hip_hdbscan.h); `min_samples == 1` needs none: core = +inf;
3. Boruvka rounds.  `comp` starts as arange(N).  A round is one `outgoing` pass (`ops.hdb_outgoing`, `sd_hdb_outgoing_f32`: the
   heaviest edge that leaves the component of every row, lowest column among equal ones), the download of `nn` and `best` (8 bytes a
   row: the round's one host synchronisation), and on the host: every component keeps its smallest edge under the total order
   (`best` descending, min(i, nn) ascending, max(i, nn) ascending), duplicates are dropped, the new components are the connected
   components of the chosen edges, numbered by lowest member, and `comp` goes up again.  The kernel's lowest column among equal
   weights IS the minimum of that order within a row, and w is exactly symmetric, so the chosen edges never close a cycle: N - 1 edges
   after at most ceil(log2 N) rounds (asserted);
4. the edges as scikit-learn's `MST_edge_dtype` with f64 distances: "euclidean" sqrt(max(0, 2 - 2 w)), "cosine" max(0, 1 - w) (what
   `cluster.cluster_hdbscan` feeds its clusterer as a precomputed matrix);
5. labels from `_process_mst` and `tree_to_labels(..., "eom", allow_single_cluster, 0.0, None)`, private functions of
   scikit-learn 1.7.2 imported in `_sklearn_tree()` alone (`labelling="sklearn"`, the default), or on the device
   (`labelling="device"`: `operator.tree_labels`, `sd_tree_labels_grouped` of include/sd_hip_tree.h: the edges of all recordings go
   up in one copy, one launch labels them with one workgroup per recording, one read brings `labels` and `bad` back, and
   scikit-learn is not imported).  The device labels are scikit-learn's on the STABLY sorted edge list; where no two edges of a
   recording have the same distance that is `_process_mst`'s own order and the two labellings are equal, and where distances tie
   `_process_mst`'s unstable argsort is platform-dependent (the last paragraph below) and the stable order is what this route defines.

The operator is injectable (`operator=`): an object with `device`, `normalise(X)`, `core(rows, k)` and `outgoing(rows, core, comp)`
over torch tensors; optionally `tree_labels(lo, hi, dist, first_edge, max_edges, min_cluster_size, allow_single_cluster) ->
(labels, bad)` (what `labelling="device"` calls: int32 edge ends counted from each recording's first row, f64 distances, int32
first_edge [G + 1] -> int32 labels [E + G], the rows of recording g from first_edge[g] + g on, and int32 bad [G]).  `DeviceRows` is
the product one; the tests run the same driver on the CPU against a numpy operator.  There is no implicit CPU route: without an
operator a host tensor raises the product path's RuntimeError.

Many recordings at once: `hdbscan_rows_groups` (one grouped core pass, one Boruvka loop over the rows of all recordings; an operator
for it also has `core_grouped(rows, k, group, max_group) -> (core, bad)` and `outgoing_grouped(rows, core, comp, group, max_group) ->
(nn, best, bad)`), `HdbscanGpuClusterer.fit_predict_many`, `cluster.cluster_hdbscan_two_stage_many`, `anti_stick_diarize.diarize_many`.

Two differences from the host route
* the host works on f64 distances (of f32 or f64 rows); here a weight is an f32 dot product of f32 unit rows, about 1e-7 away;
* equal partitions are a property of inputs without ties among the weights the tree compares, not a guarantee.  Near-ties (two
  competing weights within that rounding) are one kind.  EXACT ties are the commoner kind and have nothing to do with precision: for
  min_samples >= 3 every edge at a row whose neighbours have larger core values weighs core[i], so an outlier often hangs on the tree
  by several edges of one and the same weight, in float64 as in f32.  Which of them scikit-learn's unstable argsort hands to its linkage
  routine first depends on the order of the edge list, i.e. on who built the tree, and can decide whether the row ends as noise.  On
  record: `planted(1000, 8, 0.8, seed 2, 20 outliers)` of tests/helpers/hdbscan_ref.py, whose row 2 differs from the host at
  (6, 3, False) under both metrics and at (5, None, True) and (15, 5, True) under "cosine"; the other 45 of the 48 planted
  combinations tried agree.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import ops
from .device_rows import DeviceRoute, operator_for, upload_rows

SKLEARN_WRITTEN_AGAINST = "1.7.2"


def _sklearn_tree():
    """(MST_edge_dtype, _process_mst, tree_to_labels): the one place the private scikit-learn names are imported."""
    try:
        from sklearn.cluster._hdbscan._tree import tree_to_labels
        from sklearn.cluster._hdbscan.hdbscan import MST_edge_dtype, _process_mst
    except ImportError as e:
        raise ImportError("hdbscan_gpu labels its spanning tree with sklearn.cluster._hdbscan.hdbscan._process_mst and "
                          f"sklearn.cluster._hdbscan._tree.tree_to_labels, private functions of scikit-learn {SKLEARN_WRITTEN_AGAINST} "
                          "(the version this was written against); the installed scikit-learn does not have them") from e
    return MST_edge_dtype, _process_mst, tree_to_labels


class DeviceRows(DeviceRoute):
    """The two kernels of include/sd_hip_hdbscan.h over unit rows that live on the GPU; the workspace is kept between calls."""
    route = "HDBSCAN"

    def core(self, rows: torch.Tensor, k: int) -> torch.Tensor:
        return ops.hdb_core(rows, k, ws=self.ws)

    def outgoing(self, rows: torch.Tensor, core: torch.Tensor, comp: torch.Tensor):
        return ops.hdb_outgoing(rows, core, comp, ws=self.ws)

    def core_grouped(self, rows: torch.Tensor, k: int, group: torch.Tensor, max_group: int):
        return ops.hdb_core_grouped(rows, k, group, max_group, ws=self.ws)

    def outgoing_grouped(self, rows: torch.Tensor, core: torch.Tensor, comp: torch.Tensor, group: torch.Tensor, max_group: int):
        return ops.hdb_outgoing_grouped(rows, core, comp, group, max_group, ws=self.ws)

    def tree_labels(self, lo: torch.Tensor, hi: torch.Tensor, dist: torch.Tensor, first_edge: torch.Tensor, max_edges: int,
                    min_cluster_size: int, allow_single_cluster: bool):
        return ops.tree_labels_grouped(lo, hi, dist, first_edge, max_edges, min_cluster_size, allow_single_cluster, ws=self.ws)


def _by_lowest_member(comp: np.ndarray) -> np.ndarray:
    """The same partition with ids 0, 1, ... in the order of each component's lowest row."""
    comp = comp.reshape(-1)
    if comp.size and comp.min() >= 0 and comp.max() < 4 * comp.size:      # dense ids (what connected_components hands out): no sort of the rows
        first = np.full(int(comp.max()) + 1, comp.size, dtype=np.int64)
        np.minimum.at(first, comp, np.arange(comp.size, dtype=np.int64))
        present = np.flatnonzero(first < comp.size)
        rank = np.empty(first.size, dtype=np.int64)
        rank[present[np.argsort(first[present], kind="stable")]] = np.arange(present.size)
        return rank[comp]
    _, first, inverse = np.unique(comp, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    return rank[inverse.reshape(-1)]


def _component_edges(comp: np.ndarray, nn: np.ndarray, best: np.ndarray, rows: np.ndarray | None = None):
    """The edge each component keeps: the first under (best descending, min(i, nn) ascending, max(i, nn) ascending); an edge two
    components both chose is kept once -> (lo, hi, weight), in ascending (lo, hi).  `comp` holds ids in [0, number of components).
    `rows`: the rows that have an edge at all (the grouped driver: a row whose component is its whole recording has none); every row
    when None.  Two reductions per component instead of a sort of all rows: the heaviest weight, then the lowest (lo, hi) among the
    rows that attain it."""
    n = comp.size
    i = np.arange(n, dtype=np.int64) if rows is None else rows.astype(np.int64)
    c, w = comp[i], best[i]
    j = nn[i].astype(np.int64)
    key = np.minimum(i, j) * n + np.maximum(i, j)
    top = np.full(int(c.max()) + 1 if c.size else 0, -np.inf, dtype=best.dtype)
    np.maximum.at(top, c, w)
    at = np.flatnonzero(w == top[c])                               # one row per component unless weights tie
    lowest = np.full(top.size, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(lowest, c[at], key[at])
    at = at[key[at] == lowest[c[at]]]                              # exactly one row per component: an edge leaves a component at one of its ends
    key, keep = np.unique(key[at], return_index=True)
    return key // n, key % n, w[at[keep]]


def spanning_edges(rows: torch.Tensor, core: torch.Tensor, operator, info: dict | None = None):
    """Boruvka over `operator.outgoing` -> (lo int64 [N - 1], hi int64 [N - 1], w f32 [N - 1]): a maximum spanning tree of
    w(i, j) = min(core[i], core[j], <rows[i], rows[j]>)."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    N = rows.shape[0]
    dev = operator.device
    comp = np.arange(N, dtype=np.int64)
    n_comp = N
    los, his, ws = [], [], []
    max_rounds = max(1, math.ceil(math.log2(N)))
    rounds = 0
    while n_comp > 1:
        assert rounds < max_rounds, f"{rounds} Boruvka rounds over {N} rows: the weights are not symmetric"
        nn, best = operator.outgoing(rows, core, torch.from_numpy(comp.astype(np.int32)).to(dev))
        nn, best = nn.cpu().numpy(), best.cpu().numpy()            # the host synchronisation of the round
        if not (nn >= 0).all():                                     # -1 would index the last row below
            raise RuntimeError("a row of a partial forest has no outgoing edge: the operator's component mask is wrong")
        lo, hi, w = _component_edges(comp, nn, best)
        graph = coo_matrix((np.ones(lo.size, dtype=np.int8), (comp[lo], comp[hi])), shape=(n_comp, n_comp))
        n_next, merged = connected_components(graph, directed=False)
        assert n_comp - n_next == lo.size, "the chosen edges close a cycle: the weights are not symmetric"
        comp = _by_lowest_member(merged[comp])
        n_comp = n_next
        rounds += 1
        los.append(lo), his.append(hi), ws.append(w)
        if info is not None:
            info["rounds"] = rounds
            info["gram_rows"] += N * N
            info["components_per_round"].append(int(n_comp))
    lo, hi, w = (np.concatenate(a) for a in (los, his, ws))
    assert lo.size == N - 1, f"{lo.size} edges span {N} rows"
    return lo, hi, w


LABELLINGS = ("sklearn", "device")


def _check_labelling(labelling: str, operator) -> None:
    if labelling not in LABELLINGS:
        raise ValueError(f"labelling must be one of {LABELLINGS}, got {labelling!r}")
    if labelling == "device" and not hasattr(operator, "tree_labels"):
        raise TypeError(f"labelling='device' needs an operator with tree_labels(...); {type(operator).__name__} has none")


def _tree_distances(w: np.ndarray, metric: str) -> np.ndarray:
    """Step 4: the f64 distances of the tree's f32 weights."""
    w = w.astype(np.float64)
    return np.sqrt(np.maximum(0.0, 2.0 - 2.0 * w)) if metric == "euclidean" else np.maximum(0.0, 1.0 - w)


def _labels_on_device(trees, min_cluster_size, allow_single_cluster, metric, operator, names=None):
    """Step 5 on the device for the spanning trees [(lo, hi, w)] of recordings of two rows or more -> ([labels], [the tree's f64
    weight]).  One upload (the distances, both ends and `first_edge` in one buffer), one `operator.tree_labels`, one read of labels and
    `bad`; a recording whose `bad` is set raises RuntimeError naming it (`names`: what to call each, its position when None)."""
    counts = np.array([len(w) for _, _, w in trees], dtype=np.int64)
    E, G = int(counts.sum()), len(trees)
    dists = [_tree_distances(w, metric) for _, _, w in trees]
    buf = np.empty(4 * E + G + 1, dtype=np.int32)                  # f64 [E] | lo [E] | hi [E] | first_edge [G + 1]
    buf[:2 * E].view(np.float64)[:] = np.concatenate(dists)
    buf[2 * E:3 * E] = np.concatenate([lo for lo, _, _ in trees])
    buf[3 * E:4 * E] = np.concatenate([hi for _, hi, _ in trees])
    buf[4 * E:] = np.concatenate([[0], np.cumsum(counts)])
    up = torch.from_numpy(buf).to(operator.device)
    labels, bad = operator.tree_labels(up[2 * E:3 * E], up[3 * E:4 * E], up[:2 * E].view(torch.float64), up[4 * E:], int(counts.max()),
                                       int(min_cluster_size), bool(allow_single_cluster))
    got = torch.cat([labels, bad]).cpu().numpy()                   # the one read
    labels, bad = got[:E + G], got[E + G:]
    if bad.any():
        g = int(np.flatnonzero(bad)[0])
        raise RuntimeError(f"recording {g if names is None else names[g]}: its {int(counts[g])} edges are not a spanning tree of its "
                           f"{int(counts[g]) + 1} rows with finite distances >= 0 (sd_tree_labels_grouped reported bad={int(bad[g])})")
    starts = np.concatenate([[0], np.cumsum(counts)])[:-1] + np.arange(G)
    return [labels[a:a + c + 1].astype(int) for a, c in zip(starts, counts)], [float(d.sum()) for d in dists]


def hdbscan_rows(X, min_cluster_size: int = 2, min_samples: int | None = None, allow_single_cluster: bool = True,
                 metric: str = "euclidean", *, operator=None, return_info: bool = False, labelling: str = "sklearn"):
    """`HDBSCAN(min_cluster_size, min_samples, allow_single_cluster, metric).fit_predict` of scikit-learn from the rows X [N, D]
    themselves -> labels int [N], -1 for noise.  metric "euclidean": X holds unit rows (what the reference's call sites pass; a row
    whose norm is not within 1e-3 of 1 raises ValueError: a zero row has no cosine equivalent of its Euclidean distance);
    metric "cosine": any rows, the result is that of the host clusterer on the precomputed matrix 1 - cosine_similarity(X).
    info = {"rounds": Boruvka rounds, "gram_rows": sum of n^2 over every pass (the core pass included), "components_per_round",
    "mst_weight": the sum of the tree's f64 distances}.  labelling: "sklearn" (scikit-learn's private routines on the host) or "device"
    (`operator.tree_labels`; scikit-learn is not imported; the module's step 5).

    N = 0 and N = 1 return early as the host glue does.  min_samples > N, min_cluster_size < 2, a metric other than the two and a
    non-finite row raise ValueError before anything is launched."""
    info = {"rounds": 0, "gram_rows": 0, "components_per_round": [], "mst_weight": 0.0}
    if metric not in ("euclidean", "cosine"):
        raise ValueError(f"hdbscan_rows clusters rows under metric 'euclidean' or 'cosine'; metric={metric!r} has no rows to work on")
    operator = operator_for(X, operator, DeviceRows)
    _check_labelling(labelling, operator)
    X = torch.as_tensor(X)
    if X.dim() != 2:
        raise ValueError(f"rows must be a matrix [N, D], got {tuple(X.shape)}")
    if int(min_cluster_size) < 2:
        raise ValueError(f"min_cluster_size must be at least 2, got {min_cluster_size}")
    min_cluster_size = int(min_cluster_size)
    min_samples = min_cluster_size if min_samples is None else int(min_samples)
    if min_samples < 1:
        raise ValueError(f"min_samples must be at least 1, got {min_samples}")
    N = X.shape[0]
    if N <= 1:
        labels = np.zeros(N, dtype=int)
        return (labels, info) if return_info else labels
    if min_samples > N:
        raise ValueError(f"min_samples ({min_samples}) must be at most the number of rows ({N})")
    if X.shape[1] == 0 or not bool(torch.isfinite(X).all()):
        raise ValueError("rows must be finite and have at least one column")
    if metric == "euclidean":
        off = float((torch.linalg.vector_norm(X.double(), dim=1) - 1.0).abs().max())
        if off > 1e-3:
            raise ValueError(f"metric 'euclidean' takes unit rows (a norm is {off:.3g} away from 1); pass metric='cosine' for other rows")
    sk = _sklearn_tree() if labelling == "sklearn" else None
    dev = operator.device
    rows = operator.normalise(X.to(dev).float())
    if min_samples == 1:
        core = torch.full((N,), float("inf"), dtype=torch.float32, device=dev)
    else:
        core = operator.core(rows, min_samples - 1)
        info["gram_rows"] += N * N
    lo, hi, w = spanning_edges(rows, core, operator, info)
    if labelling == "device":
        (labels,), (info["mst_weight"],) = _labels_on_device([(lo, hi, w)], min_cluster_size, allow_single_cluster, metric, operator)
    else:
        labels, info["mst_weight"] = _labels_of_tree(lo, hi, w, N, min_cluster_size, allow_single_cluster, metric, sk)
    return (labels, info) if return_info else labels


def _labels_of_tree(lo, hi, w, n, min_cluster_size, allow_single_cluster, metric, sk):
    """Labels of the n rows whose maximum spanning tree of w is (lo, hi, w), by scikit-learn's routines -> (labels, the tree's f64
    weight): steps 4 and 5 of the module's list."""
    MST_edge_dtype, process_mst, tree_to_labels = sk
    dist = _tree_distances(w, metric)
    mst = np.empty(n - 1, dtype=MST_edge_dtype)
    mst["current_node"], mst["next_node"], mst["distance"] = lo, hi, dist
    labels = tree_to_labels(process_mst(mst), min_cluster_size, "eom", bool(allow_single_cluster), 0.0, None)[0]
    return np.asarray(labels).astype(int), float(dist.sum())


def _shared_tiles(group: np.ndarray):
    """(tiles on the diagonal, tiles above it whose row block and column block share a group) of the 128 x 128 tiling of the rows: what
    the grouped passes do not skip.  The outgoing pass computes the first plus the second, the core pass the first plus twice the second."""
    T = -(-group.size // 128)
    first, last = group[::128], group[np.minimum(np.arange(T) * 128 + 127, group.size - 1)]
    above = np.searchsorted(first, last, side="right") - (np.arange(T) + 1)             # the J > I with group[first row of J] == group[last row of I]
    return T, int(np.maximum(above, 0).sum())


def spanning_edges_groups(rows: torch.Tensor, core: torch.Tensor, sizes, operator, info: dict | None = None, core_bad=None):
    """`spanning_edges` for many recordings in one Boruvka loop: rows [N, d] holds the rows of all recordings one after another, `sizes`
    the rows of each -> a list with one (lo, hi, w) per recording, indices counted from the recording's first row: exactly the edge list
    `spanning_edges` builds for that recording alone (the module's docstring has the argument).  One `operator.outgoing_grouped` pass
    and one host read per round; `bad` (and `core_bad`, the verdict of the grouped core pass, in the first round) comes back in the
    same read."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    sizes = np.asarray(sizes, dtype=np.int64)
    N = int(sizes.sum())
    dev = operator.device
    max_group = int(sizes.max(initial=0))
    group_h = np.repeat(np.arange(sizes.size, dtype=np.int32), sizes)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    size_of_row = sizes[group_h]
    group = torch.from_numpy(group_h).to(dev)
    comp = np.arange(N, dtype=np.int64)
    n_comp, n_groups = N, int((sizes > 0).sum())
    los, his, ws = [], [], []
    max_rounds = max(1, math.ceil(math.log2(max(max_group, 1))))
    rounds = 0
    while n_comp > n_groups:
        assert rounds < max_rounds, f"{rounds} Boruvka rounds over recordings of at most {max_group} rows: the weights are not symmetric"
        nn, best, bad = operator.outgoing_grouped(rows, core, torch.from_numpy(comp.astype(np.int32)).to(dev), group, max_group)
        parts = [nn, best.view(torch.int32), bad.reshape(1)] + ([core_bad.reshape(1)] if core_bad is not None else [])
        got = torch.cat(parts).cpu().numpy()                       # the host synchronisation of the round
        nn, best, broken = got[:N], got[N:2 * N].view(np.float32), bool(got[2 * N:].any())
        core_bad = None
        if broken:
            raise RuntimeError(f"grouped pass over {N} rows: `group` decreases or a group exceeds max_group={max_group}")
        has = np.flatnonzero(nn >= 0)                              # a row whose component is its whole recording has no edge and is left out
        whole = np.bincount(comp, minlength=n_comp)[comp] == size_of_row      # rows whose component is their whole recording
        if not np.array_equal(nn < 0, whole):
            raise RuntimeError("a row has no outgoing edge although its recording is not one component yet, or has one although it "
                               "is: the operator's group or component mask is wrong")
        lo, hi, w = _component_edges(comp, nn, best, has)
        graph = coo_matrix((np.ones(lo.size, dtype=np.int8), (comp[lo], comp[hi])), shape=(n_comp, n_comp))
        n_next, merged = connected_components(graph, directed=False)
        assert n_comp - n_next == lo.size, "the chosen edges close a cycle: the weights are not symmetric"
        comp = _by_lowest_member(merged[comp])
        n_comp = n_next
        rounds += 1
        los.append(lo), his.append(hi), ws.append(w)
        if info is not None:
            info["rounds"] = rounds
            info["components_per_round"].append(int(n_comp))
    if not los:
        los, his, ws = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
    lo, hi, w = (np.concatenate(a) for a in (los, his, ws))
    rec = group_h[lo].astype(np.int64)
    assert np.array_equal(rec, group_h[hi]), "an edge joins two recordings: the operator's group mask is wrong"
    order = np.argsort(rec, kind="stable")                          # within a recording the order stays (round, lo, hi)
    lo, hi, w, rec = lo[order], hi[order], w[order], rec[order]
    cuts = np.searchsorted(rec, np.arange(sizes.size + 1))
    assert np.array_equal(np.diff(cuts), np.maximum(sizes - 1, 0)), "a recording's edges do not span it"
    return [(lo[a:b] - off, hi[a:b] - off, w[a:b]) for a, b, off in zip(cuts[:-1], cuts[1:], offsets[:-1])]


def hdbscan_rows_groups(X, sizes, min_cluster_size: int = 2, min_samples: int | None = None, allow_single_cluster: bool = True,
                        metric: str = "euclidean", *, operator=None, return_info: bool = False, labelling: str = "sklearn"):
    """`hdbscan_rows` for many recordings in one driver: X [N, D] holds the rows of all recordings one after another, `sizes` the number
    of rows of each (0 and 1 are legal and return as the host glue does) -> a list with one label array per recording, equal to
    `hdbscan_rows` on that recording's rows alone, exactly.  labelling as for `hdbscan_rows`; "device" labels ALL recordings in one
    launch (one upload of the edges, one read of labels and `bad`; a recording whose `bad` is set raises RuntimeError naming it).

    A row's core value and every tree edge look only inside the row's own recording, so ONE grouped core pass
    (`operator.core_grouped`, `sd_hdb_core_grouped_f32`) and ONE Boruvka loop (`operator.outgoing_grouped`,
    `sd_hdb_outgoing_grouped_f32`: one pass and one host read per round) serve all recordings; the rounds are the maximum over the
    recordings, at most ceil(log2(max(sizes))) (asserted), not their sum.  Why the labels are equal with no condition on ties: per
    recording the grouped entries return the `core`, the `nn` (minus the recording's first row) and the bits of `best` of the
    ungrouped ones on its rows alone (include/sd_hip_hdbscan.h); by induction over the rounds every recording's components are those
    of its lone run, a round keeps the same edge per component (the order (best, lo, hi) does not change when every index moves by
    the same offset) and lists them in ascending (lo, hi); so a recording's edges, taken out in (round, lo, hi) order with its offset
    subtracted, ARE the array `spanning_edges` builds for it alone, and the same array goes into the same scikit-learn routines.

    A non-finite row, a row that is not a unit row under "euclidean", and `min_samples` above a recording's size (sizes >= 2) raise
    ValueError naming the recording before anything is launched.  `bad` of the kernels (a broken promise about `group`) raises
    RuntimeError.  info = {"rounds", "components_per_round" (over all rows), "gram_tiles": the 128 x 128 tiles the passes did not skip,
    "gram_tiles_per_pass", "mst_weight": per recording}; the tile counts are computed on the host and only when info is asked for."""
    if metric not in ("euclidean", "cosine"):
        raise ValueError(f"hdbscan_rows_groups clusters rows under metric 'euclidean' or 'cosine'; metric={metric!r} has no rows to work on")
    sizes = [int(s) for s in sizes]
    info = {"rounds": 0, "components_per_round": [], "gram_tiles": 0, "gram_tiles_per_pass": [], "mst_weight": [0.0] * len(sizes)}
    operator = operator_for(X, operator, DeviceRows)
    _check_labelling(labelling, operator)
    X = torch.as_tensor(X)
    if X.dim() != 2:
        raise ValueError(f"rows must be a matrix [N, D], got {tuple(X.shape)}")
    if int(min_cluster_size) < 2:
        raise ValueError(f"min_cluster_size must be at least 2, got {min_cluster_size}")
    min_cluster_size = int(min_cluster_size)
    min_samples = min_cluster_size if min_samples is None else int(min_samples)
    if min_samples < 1:
        raise ValueError(f"min_samples must be at least 1, got {min_samples}")
    N = X.shape[0]
    if min(sizes, default=0) < 0 or sum(sizes) != N:
        raise ValueError(f"sizes {sizes} do not add up to the {N} rows")
    labels = [np.zeros(s, dtype=int) for s in sizes]                # what sizes 0 and 1 keep
    if max(sizes, default=0) <= 1:
        return (labels, info) if return_info else labels
    for g, s in enumerate(sizes):
        if s >= 2 and min_samples > s:
            raise ValueError(f"recording {g}: min_samples ({min_samples}) must be at most the number of rows ({s})")
    if X.shape[1] == 0:
        raise ValueError("rows must be finite and have at least one column")
    group_h = np.repeat(np.arange(len(sizes)), sizes)
    finite = torch.isfinite(X).all(dim=1)
    if not bool(finite.all()):
        row = int(torch.nonzero(~finite)[0])
        raise ValueError(f"recording {int(group_h[row])}: rows must be finite (row {row} of all rows is not)")
    if metric == "euclidean":
        off = (torch.linalg.vector_norm(X.double(), dim=1) - 1.0).abs()
        in_play = torch.from_numpy(np.asarray(sizes)[group_h] >= 2).to(off.device)     # a lone row is never looked at, as in hdbscan_rows
        off = torch.where(in_play, off, torch.zeros_like(off))
        if float(off.max()) > 1e-3:
            row = int(off.argmax())
            raise ValueError(f"recording {int(group_h[row])}: metric 'euclidean' takes unit rows (a norm is {float(off[row]):.3g} away "
                             "from 1); pass metric='cosine' for other rows")
    sk = _sklearn_tree() if labelling == "sklearn" else None
    dev = operator.device
    rows = operator.normalise(X.to(dev).float())
    max_group = max(sizes)
    core_bad = None
    if min_samples == 1:
        core = torch.full((N,), float("inf"), dtype=torch.float32, device=dev)
    else:
        group = torch.from_numpy(group_h.astype(np.int32)).to(dev)
        core, core_bad = operator.core_grouped(rows, min_samples - 1, group, max_group)
    edges = spanning_edges_groups(rows, core, sizes, operator, info, core_bad)
    if labelling == "device":
        which = [g for g, s in enumerate(sizes) if s >= 2]
        got, weights = _labels_on_device([edges[g] for g in which], min_cluster_size, allow_single_cluster, metric, operator, names=which)
        for g, lab, weight in zip(which, got, weights):
            labels[g], info["mst_weight"][g] = lab, weight
    else:
        for g, (s, (lo, hi, w)) in enumerate(zip(sizes, edges)):
            if s >= 2:
                labels[g], info["mst_weight"][g] = _labels_of_tree(lo, hi, w, s, min_cluster_size, allow_single_cluster, metric, sk)
    if return_info:
        diagonal, above = _shared_tiles(group_h)
        info["gram_tiles_per_pass"] = ([diagonal + 2 * above] if min_samples > 1 else []) + [diagonal + above] * info["rounds"]
        info["gram_tiles"] = sum(info["gram_tiles_per_pass"])
    return (labels, info) if return_info else labels


class HdbscanGpuClusterer:
    """A scikit-learn `HDBSCAN` stand-in on the device route, for the `clusterer_factory=` argument of
    `cluster.cluster_hdbscan_two_stage`: `fit_predict` takes L2-normalised rows (metric "euclidean") or any rows (metric "cosine").
    A "precomputed" distance matrix raises ValueError: the route needs the rows, not a matrix.  labelling: as for `hdbscan_rows`."""

    def __init__(self, min_cluster_size: int = 2, min_samples: int | None = None, allow_single_cluster: bool = True,
                 metric: str = "euclidean", operator=None, labelling: str = "sklearn"):
        if metric not in ("euclidean", "cosine"):
            raise ValueError(f"HdbscanGpuClusterer clusters rows (metric 'euclidean' or 'cosine'); metric={metric!r} has no rows to work on")
        self.min_cluster_size = min_cluster_size
        self.min_samples = min_samples
        self.allow_single_cluster = allow_single_cluster
        self.metric = metric
        if labelling not in LABELLINGS:
            raise ValueError(f"labelling must be one of {LABELLINGS}, got {labelling!r}")
        self.operator = operator
        self.labelling = labelling

    @classmethod
    def factory(cls, operator=None, labelling: str = "sklearn"):
        return lambda **kw: cls(kw.get("min_cluster_size", 2), kw.get("min_samples"), kw.get("allow_single_cluster", True),
                                kw.get("metric", "euclidean"), operator=operator, labelling=labelling)

    def fit_predict(self, X) -> np.ndarray:
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
        if self.operator is None:
            X = upload_rows(X, "HdbscanGpuClusterer runs on the HIP path (a visible GPU); there is no CPU fallback")
        return hdbscan_rows(X, self.min_cluster_size, self.min_samples, self.allow_single_cluster, self.metric, operator=self.operator,
                            labelling=self.labelling)

    def fit_predict_many(self, list_of_X) -> list:
        """`fit_predict` of every matrix of the list (all of one width) through ONE grouped driver (`hdbscan_rows_groups`) -> a list of
        label arrays, each equal to `fit_predict` on its matrix alone."""
        mats = [np.ascontiguousarray(X, dtype=np.float32) for X in list_of_X]
        if not mats:
            return []
        widths = {m.shape[1] for m in mats if m.ndim == 2}
        if any(m.ndim != 2 for m in mats) or len(widths) != 1:
            raise ValueError(f"fit_predict_many takes matrices [n, D] of one width, got {[m.shape for m in mats]}")
        X = torch.from_numpy(np.concatenate(mats))
        if self.operator is None:
            X = upload_rows(X, "HdbscanGpuClusterer runs on the HIP path (a visible GPU); there is no CPU fallback")
        return hdbscan_rows_groups(X, [len(m) for m in mats], self.min_cluster_size, self.min_samples, self.allow_single_cluster, self.metric,
                                   operator=self.operator, labelling=self.labelling)
