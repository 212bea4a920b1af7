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
   scikit-learn 1.7.2 imported in `_sklearn_tree()` alone.

The operator is injectable (`operator=`): an object with `device`, `normalise(X)`, `core(rows, k)` and `outgoing(rows, core, comp)`
over torch tensors.  `DeviceRows` is the product one; the tests run the same driver on the CPU against a numpy operator.  There is no
implicit CPU route: without an operator a host tensor raises the product path's RuntimeError.

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


def _by_lowest_member(comp: np.ndarray) -> np.ndarray:
    """The same partition with ids 0, 1, ... in the order of each component's lowest row."""
    _, first, inverse = np.unique(comp, return_index=True, return_inverse=True)
    rank = np.empty(first.size, dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.size)
    return rank[inverse.reshape(-1)]


def _component_edges(comp: np.ndarray, nn: np.ndarray, best: np.ndarray):
    """The edge each component keeps: the first under (best descending, min(i, nn) ascending, max(i, nn) ascending); an edge two
    components both chose is kept once -> (lo, hi, weight)."""
    i = np.arange(comp.size, dtype=np.int64)
    nn = nn.astype(np.int64)
    lo, hi = np.minimum(i, nn), np.maximum(i, nn)
    order = np.lexsort((hi, lo, -best, comp))                      # the last key is the primary one
    c_sorted = comp[order]
    first = order[np.concatenate(([True], c_sorted[1:] != c_sorted[:-1]))]
    _, keep = np.unique(lo[first] * comp.size + hi[first], return_index=True)
    first = first[keep]
    return lo[first], hi[first], best[first]


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


def hdbscan_rows(X, min_cluster_size: int = 2, min_samples: int | None = None, allow_single_cluster: bool = True,
                 metric: str = "euclidean", *, operator=None, return_info: bool = False):
    """`HDBSCAN(min_cluster_size, min_samples, allow_single_cluster, metric).fit_predict` of scikit-learn from the rows X [N, D]
    themselves -> labels int [N], -1 for noise.  metric "euclidean": X holds unit rows (what the reference's call sites pass; a row
    whose norm is not within 1e-3 of 1 raises ValueError: a zero row has no cosine equivalent of its Euclidean distance);
    metric "cosine": any rows, the result is that of the host clusterer on the precomputed matrix 1 - cosine_similarity(X).
    info = {"rounds": Boruvka rounds, "gram_rows": sum of n^2 over every pass (the core pass included), "components_per_round",
    "mst_weight": the sum of the tree's f64 distances}.

    N = 0 and N = 1 return early as the host glue does.  min_samples > N, min_cluster_size < 2, a metric other than the two and a
    non-finite row raise ValueError before anything is launched."""
    info = {"rounds": 0, "gram_rows": 0, "components_per_round": [], "mst_weight": 0.0}
    if metric not in ("euclidean", "cosine"):
        raise ValueError(f"hdbscan_rows clusters rows under metric 'euclidean' or 'cosine'; metric={metric!r} has no rows to work on")
    operator = operator_for(X, operator, DeviceRows)
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
    MST_edge_dtype, process_mst, tree_to_labels = _sklearn_tree()
    dev = operator.device
    rows = operator.normalise(X.to(dev).float())
    if min_samples == 1:
        core = torch.full((N,), float("inf"), dtype=torch.float32, device=dev)
    else:
        core = operator.core(rows, min_samples - 1)
        info["gram_rows"] += N * N
    lo, hi, w = spanning_edges(rows, core, operator, info)
    w = w.astype(np.float64)
    dist = np.sqrt(np.maximum(0.0, 2.0 - 2.0 * w)) if metric == "euclidean" else np.maximum(0.0, 1.0 - w)
    mst = np.empty(N - 1, dtype=MST_edge_dtype)
    mst["current_node"], mst["next_node"], mst["distance"] = lo, hi, dist
    info["mst_weight"] = float(dist.sum())
    labels = tree_to_labels(process_mst(mst), min_cluster_size, "eom", bool(allow_single_cluster), 0.0, None)[0]
    labels = np.asarray(labels).astype(int)
    return (labels, info) if return_info else labels


class HdbscanGpuClusterer:
    """A scikit-learn `HDBSCAN` stand-in on the device route, for the `clusterer_factory=` argument of
    `cluster.cluster_hdbscan_two_stage`: `fit_predict` takes L2-normalised rows (metric "euclidean") or any rows (metric "cosine").
    A "precomputed" distance matrix raises ValueError: the route needs the rows, not a matrix."""

    def __init__(self, min_cluster_size: int = 2, min_samples: int | None = None, allow_single_cluster: bool = True,
                 metric: str = "euclidean", operator=None):
        if metric not in ("euclidean", "cosine"):
            raise ValueError(f"HdbscanGpuClusterer clusters rows (metric 'euclidean' or 'cosine'); metric={metric!r} has no rows to work on")
        self.min_cluster_size = min_cluster_size
        self.min_samples = min_samples
        self.allow_single_cluster = allow_single_cluster
        self.metric = metric
        self.operator = operator

    @classmethod
    def factory(cls, operator=None):
        return lambda **kw: cls(kw.get("min_cluster_size", 2), kw.get("min_samples"), kw.get("allow_single_cluster", True),
                                kw.get("metric", "euclidean"), operator=operator)

    def fit_predict(self, X) -> np.ndarray:
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
        if self.operator is None:
            X = upload_rows(X, "HdbscanGpuClusterer runs on the HIP path (a visible GPU); there is no CPU fallback")
        return hdbscan_rows(X, self.min_cluster_size, self.min_samples, self.allow_single_cluster, self.metric, operator=self.operator)
