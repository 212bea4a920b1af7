"""Device route for the reference's clustering: average-linkage AHC on cosine distance without the N x N matrix.

`cluster.ahc_cosine` [REF diar_diag.py:218-226] copies the N x N affinity off the GPU, turns it into an f64 distance matrix and hands
it to scikit-learn.  The matrix is not needed: the average linkage between clusters A and B of unit rows is

    1 - (1 / (|A| |B|)) . sum_{a in A, b in B} <x_a, x_b>  =  1 - <s_A, s_B> / (|A| |B|),      s_A = sum of the rows of A,

so a cluster is the sum of its unit rows and its size, and a merge is one vector add.  Average linkage is reducible: merging a pair of
mutually nearest clusters never brings a third cluster closer to the merged one than it was to the nearer of the two, so EVERY pair of
mutually nearest clusters can be merged in the same round and the dendrogram is the greedy one.  The cut at cosine `cos_thr` is the set
of merges whose score is above it.  Opt-in: `diarize_audio(..., clustering="ahc_gpu")`; `cluster.py` and `clustering="ahc"` are
unchanged.

A round
* `nearest`: the best other cluster of every active cluster (`ops.ahc_nearest`, `sd_ahc_nearest_f32`, include/sd_hip_ahc.h): one
  Gram-with-argmax pass over the n_active x D sums on the f32 matrix cores, nothing n x n is stored;
* `merge`: every reciprocal pair above the threshold, into the lower index (`ops.ahc_merge`, `sd_ahc_merge_f32`);
* the number of merges is read back (the one host synchronisation of a round; 0 ends the loop);
* the sums, counts and the row-to-cluster table are compacted with torch indexing on the operator's device (plumbing, no kernel).
Merging goes into the lower index and compaction keeps order, so the final cluster ids are numbered by first appearance.

The operator is injectable (`operator=`): an object with `device`, `normalise(X)`, `nearest(sums, inv_count)` and
`merge(sums, count, inv_count, nn, best, cos_thr)` over torch tensors.  `DeviceSums` is the product one; the tests run the same driver
on the CPU against a numpy operator.  There is no implicit CPU route: without an operator a host tensor raises the product path's
RuntimeError.

Many recordings at once: `ahc_cosine_groups(X, sizes, cos_thr)` is the same loop over the rows of all recordings, with
`nearest_grouped(sums, inv_count, group, max_group) -> (nn, best, bad)` (`ops.ahc_nearest_grouped`, `sd_ahc_nearest_grouped_f32`) in
place of `nearest`: a cluster looks for its neighbour inside its own recording only, so one pass, one merge and one host
synchronisation per round serve the whole folder, and every recording gets the labels `ahc_cosine_rows` gives it alone (DESIGN
section 18).  Opt-in: `diarization_baseline.diarize_audios`, `Diarizer.diarize_many`.

Speaker-count bounds (`min_clusters=`, `max_clusters=` of both drivers; both None: everything above, unchanged).  Average linkage has
no inversions, so the partition into k clusters is the dendrogram with its N - k highest merges applied, and the bounded count is the
threshold's count clamped into [min, max].  The driver carries two more vectors per active cluster, compacted with the sums: `first`,
the cluster's lowest row counted from its recording's first row, and `height`, f32, +inf at the start.  After each `merge` every pair
(i kept, j absorbed), in ascending j, is logged as lo = first[i], hi = first[j], key = min(best[i], height[i], height[j]), and
height[i] becomes the key: the merge score, pushed down so that it never exceeds a child's key (an f32 score can exceed a child's by
an ulp, and the cut must not let that order a parent before its child).
* Phase A is the loop above at `cos_thr`: the same passes, the same merges.
* Phase B runs only for the recordings that phase A leaves with more clusters than their maximum: their active clusters are kept, all
  others dropped, and the loop goes on at a threshold of -inf until a round merges nothing, i.e. to the COMPLETE dendrogram.  Stopping
  at "<= max clusters" would be wrong: a round merges every reciprocal pair, low ones with high ones, and a higher merge of the next
  round (not logged yet) belongs before a lower one of this round (DESIGN section 22 has the six-cluster example).
* The log, sorted stably by recording (round order is kept, so children come before parents), goes to
  `cut(lo, hi, key, first_merge, first_row, cos_thr, min_clusters, max_clusters) -> (labels, clusters, bad)`, the one more method
  of the operator protocol (`ops.ahc_cut_grouped`, `sd_ahc_cut_grouped`, include/sd_hip_cut.h): one launch for all recordings picks
  each recording's merges and labels its rows.  `bad` and `clusters` come back in one host read; a bad recording raises RuntimeError.

Two differences from the host route
* the host clips 1 - K at 0 and symmetrises an f32 K; here there is no K: a score is an f32 dot product of f32 sums, and differs from
  the host's f64 mean of f32 cosines by f32 rounding, about 1e-7;
* equal partitions are therefore a property of inputs without near-ties (no merge height within that rounding of the cut or of a
  competing merge; the caveat of DESIGN section 8), not a guarantee.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .device_rows import DeviceRoute, operator_for, upload_rows


class DeviceSums(DeviceRoute):
    """The kernels of include/sd_hip_ahc.h over cluster sums that live on the GPU, and the cut of include/sd_hip_cut.h; the workspace
    is kept between calls."""
    route = "AHC"

    def nearest(self, sums: torch.Tensor, inv_count: torch.Tensor):
        return ops.ahc_nearest(sums, inv_count, ws=self.ws)

    def nearest_grouped(self, sums: torch.Tensor, inv_count: torch.Tensor, group: torch.Tensor, max_group: int):
        return ops.ahc_nearest_grouped(sums, inv_count, group, max_group, ws=self.ws)

    def merge(self, sums, count, inv_count, nn, best, cos_thr: float):
        return ops.ahc_merge(sums, count, inv_count, nn, best, cos_thr)

    def cut(self, lo, hi, key, first_merge, first_row, cos_thr: float, min_clusters, max_clusters):
        return ops.ahc_cut_grouped(lo, hi, key, first_merge, first_row, cos_thr, min_clusters, max_clusters, ws=self.ws)


NO_BOUND = 2 ** 31 - 1          # max_clusters of a recording without a maximum


def _bounds(min_clusters, max_clusters, n_groups: int):
    """The two bounds as one int per recording (a scalar serves every recording; None: 1 and NO_BOUND), or None when both are None.
    1 <= min <= max is required of every recording: ValueError."""
    if min_clusters is None and max_clusters is None:
        return None
    out = []
    for name, value, default in (("min_clusters", min_clusters, 1), ("max_clusters", max_clusters, NO_BOUND)):
        value = default if value is None else value
        per = [int(value)] * n_groups if np.ndim(value) == 0 else [int(v) for v in value]
        if len(per) != n_groups:
            raise ValueError(f"{name} has {len(per)} entries for {n_groups} recordings")
        out.append(per)
    for g, (lo, hi) in enumerate(zip(*out)):
        if not 1 <= lo <= hi <= NO_BOUND:
            raise ValueError(f"recording {g}: 1 <= min_clusters <= max_clusters is required, got min_clusters={lo} max_clusters={hi}")
    return out


def _true_indices(mask: torch.Tensor, count: int) -> torch.Tensor:
    """The `count` indices at which `mask` is set, ascending, without a data-dependent shape (the compaction's scatter)."""
    n = mask.shape[0]
    pos = torch.cumsum(mask, 0) - 1
    out = torch.empty((count + 1,), dtype=torch.long, device=mask.device)
    out.scatter_(0, torch.where(mask, pos, torch.full_like(pos, count)), torch.arange(n, device=mask.device))
    return out[:count]


def _bounded(operator, sums, sizes, cos_thr: float, bounds, grouped: bool, info: dict, want_tiles: bool = False):
    """The bounded form of both drivers (module docstring, "Speaker-count bounds") over the unit rows `sums` of recordings of `sizes`
    rows -> one label array per recording; fills `info`."""
    if not hasattr(operator, "cut"):
        raise TypeError("min_clusters / max_clusters need an operator with cut(lo, hi, key, first_merge, first_row, cos_thr, min_clusters, max_clusters)")
    dev, N, G = operator.device, sums.shape[0], len(sizes)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    max_group = max(sizes)
    count = torch.ones((N,), dtype=torch.float32, device=dev)
    inv_count = torch.ones((N,), dtype=torch.float32, device=dev)
    group = torch.from_numpy(np.repeat(np.arange(G, dtype=np.int32), sizes)).to(dev)
    first = torch.from_numpy(np.concatenate([np.arange(s, dtype=np.int32) for s in sizes])).to(dev)    # a cluster's lowest row, within its recording
    height = torch.full((N,), float("inf"), dtype=torch.float32, device=dev)
    log = []                                                                            # per round: (group, lo, hi, key) of its merges
    tiles = torch.zeros((), dtype=torch.long, device=dev)

    def rounds(sums, count, inv_count, group, first, height, thr):
        nonlocal tiles
        n, done = sums.shape[0], 0
        while True:
            if grouped:
                nn, best, bad = operator.nearest_grouped(sums, inv_count, group, max_group)
                if want_tiles:
                    tiles = tiles + _band_tiles(group, max_group)
            else:
                nn, best = operator.nearest(sums, inv_count)
                bad = torch.zeros((1,), dtype=torch.int32, device=dev)
                info["gram_rows"] += n * n
            target, n_merged = operator.merge(sums, count, inv_count, nn, best, thr)
            m, broken = torch.cat((n_merged.reshape(1), bad.reshape(1))).tolist()       # the host synchronisation of the round
            if broken:
                raise RuntimeError(f"grouped nearest pass over {n} clusters: `group` decreases or a group exceeds max_group={max_group}")
            if m == 0:
                return sums, count, inv_count, group, first, height, best, done
            done += 1
            target = target.long()
            keep = target == torch.arange(n, device=dev)
            # the log beside the compaction: every pair (i kept, j absorbed) in ascending j
            j = _true_indices(~keep, m)
            i = target[j]
            key = torch.minimum(best[i], torch.minimum(height[i], height[j]))
            log.append((group[j], first[i], first[j], key))
            height = height.index_put((i,), key)
            src = _true_indices(keep, n - m)
            sums, count, inv_count, group, first, height = sums[src], count[src], inv_count[src], group[src], first[src], height[src]
            n -= m

    # phase A: today's loop at cos_thr
    sums, count, inv_count, group, first, height, best, info["rounds"] = rounds(sums, count, inv_count, group, first, height, float(cos_thr))
    if not grouped:
        info["last_best"] = float(best.max())
    left = torch.bincount(group.long(), minlength=G).tolist()
    info["threshold_clusters"] = left
    # phase B: the rest of the dendrogram of every recording the threshold leaves above its maximum
    over = [g for g in range(G) if left[g] > bounds[1][g]]
    info["rounds_full"] = 0
    if over:
        mask = torch.zeros((G,), dtype=torch.bool, device=dev)
        mask[torch.tensor(over, device=dev)] = True
        src = _true_indices(mask[group.long()], sum(left[g] for g in over))
        state = (sums[src], count[src], inv_count[src], group[src], first[src], height[src])
        info["rounds_full"] = rounds(*state, float("-inf"))[-1]
    # the log by recording (stable: round order is kept, children stay before parents), and the cut
    if log:
        g_all, lo, hi, key = (torch.cat(parts) for parts in zip(*log))
        order = torch.sort(g_all, stable=True).indices
        g_all, lo, hi, key = g_all[order], lo[order].contiguous(), hi[order].contiguous(), key[order].contiguous()
        per = torch.bincount(g_all.long(), minlength=G)
    else:
        lo = hi = torch.zeros((0,), dtype=torch.int32, device=dev)
        key = torch.zeros((0,), dtype=torch.float32, device=dev)
        per = torch.zeros((G,), dtype=torch.long, device=dev)
    first_merge = torch.cat((torch.zeros((1,), dtype=torch.long, device=dev), torch.cumsum(per, 0))).to(torch.int32)
    first_row = torch.from_numpy(offsets.astype(np.int32)).to(dev)
    lo_b, hi_b = (torch.tensor(b, dtype=torch.int32).to(dev) for b in bounds)
    labels, clusters, bad = operator.cut(lo, hi, key, first_merge, first_row, float(cos_thr), lo_b, hi_b)
    flat = torch.cat((bad, clusters, labels)).cpu().numpy()                             # the one host read after the launch
    bad, clusters, flat = flat[:G], flat[G:2 * G], flat[2 * G:].astype(int)
    if bad.any():
        raise RuntimeError(f"bounded cut: the merge log of recording(s) {np.flatnonzero(bad).tolist()} is broken (include/sd_hip_cut.h)")
    info["clusters"] = [int(c) for c in clusters]
    if want_tiles:
        info["gram_tiles"] = int(tiles)
    return [flat[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


def ahc_cosine_rows(X, cos_thr: float = 0.70, *, operator=None, return_info: bool = False, min_clusters=None, max_clusters=None):
    """`cluster.ahc_cosine(cosine_similarity(X), cos_thr)` from the rows X [N, D] themselves -> labels int [N], numbered by first
    appearance (info = {"rounds": rounds that merged something, "clusters", "gram_rows": sum of n_active^2 over every nearest pass,
    the last one that found nothing to merge included, "last_best": the largest score of that last pass, i.e. how far the closest
    remaining pair is from the cut; -inf when one cluster is left}).

    `min_clusters` / `max_clusters` (both None: the threshold cut above, unchanged): the cluster count is the threshold's, clamped
    into [min, max] by a dendrogram cut on the device (module docstring); 1 <= min <= max, ValueError otherwise.  info then also has
    "threshold_clusters" and "rounds_full", and "clusters" is the bounded count.

    Early returns as in `cluster.ahc_cosine`: N = 0 and N = 1.  A non-finite row raises ValueError before anything is launched."""
    from . import cluster
    info = {"rounds": 0, "clusters": 0, "gram_rows": 0, "last_best": float("-inf")}
    bounds = _bounds(min_clusters, max_clusters, 1)
    operator = operator_for(X, operator, DeviceSums)
    X = torch.as_tensor(X)
    if X.dim() != 2:
        raise ValueError(f"rows must be a matrix [N, D], got {tuple(X.shape)}")
    N = X.shape[0]
    if N <= 1:
        info["clusters"] = N
        labels = np.zeros(N, dtype=int)
        return (labels, info) if return_info else labels
    if X.shape[1] == 0 or not bool(torch.isfinite(X).all()):
        raise ValueError("rows must be finite and have at least one column")
    dev = operator.device
    sums = operator.normalise(X.to(dev).float())
    if bounds is not None:
        labels, = _bounded(operator, sums, [N], cos_thr, bounds, False, info)
        for name in ("clusters", "threshold_clusters"):
            info[name] = info[name][0]
        assert np.array_equal(labels, cluster.relabel_by_first_appearance(labels)), "cluster ids are not numbered by first appearance"
        return (labels, info) if return_info else labels
    count = torch.ones((N,), dtype=torch.float32, device=dev)
    inv_count = torch.ones((N,), dtype=torch.float32, device=dev)
    cluster_of = torch.arange(N, device=dev)                        # row -> index of its cluster among the active ones
    n = N
    while True:
        nn, best = operator.nearest(sums, inv_count)
        info["gram_rows"] += n * n
        target, n_merged = operator.merge(sums, count, inv_count, nn, best, float(cos_thr))
        m = int(n_merged)                                           # the host synchronisation of the round
        if m == 0:
            info["last_best"] = float(best.max())
            break
        info["rounds"] += 1
        # compaction without a data-dependent shape (m is known): kept rows in order, the others dumped into one slot past the end
        target = target.long()
        ids = torch.arange(n, device=dev)
        keep = target == ids
        new_id = torch.cumsum(keep, 0) - 1
        cluster_of = new_id[target[cluster_of]]
        src = torch.empty((n - m + 1,), dtype=torch.long, device=dev)
        src.scatter_(0, torch.where(keep, new_id, torch.full_like(new_id, n - m)), ids)
        src = src[: n - m]
        sums, count, inv_count = sums[src], count[src], inv_count[src]
        n -= m
    labels = cluster_of.cpu().numpy().astype(int)
    assert np.array_equal(labels, cluster.relabel_by_first_appearance(labels)), "cluster ids are not numbered by first appearance"
    info["clusters"] = n
    return (labels, info) if return_info else labels


TILE = 128          # the tile edge of the nearest kernels (GT_T of csrc/sd_gram_tile.h), for the count of `gram_tiles`


def _band_tiles(group: torch.Tensor, max_group: int) -> torch.Tensor:
    """The tiles one grouped nearest pass computes (a 0-dim tensor on the device of `group`): every diagonal tile, and tile (I, J),
    0 < J - I <= W, whose row block and column block share a group: group[last row of I] == group[first row of J].  The first rows of
    the blocks ascend, so for a row block these J are a run that starts at I + 1: one searchsorted finds its end."""
    n = group.shape[0]
    T = -(-n // TILE)
    W = min(T - 1, -(-(max_group - 1) // TILE))
    if W == 0:
        return torch.tensor(T, device=group.device)
    first = group[::TILE].contiguous()                                                  # [T]
    last = group[TILE - 1::TILE][:T - 1].contiguous()                                   # [T - 1]: the last block has no block to its right
    blocks = torch.arange(T - 1, device=group.device)
    run = torch.searchsorted(first, last, right=True) - (blocks + 1)
    return T + torch.minimum(run, (T - 1 - blocks).clamp(max=W)).clamp(min=0).sum()


def ahc_cosine_groups(X, sizes, cos_thr: float = 0.70, *, operator=None, return_info: bool = False, min_clusters=None, max_clusters=None):
    """`ahc_cosine_rows` for many recordings in one driver: X [N, D] holds the rows of all recordings one after another, `sizes` the
    number of rows of each (0 and 1 are legal) -> a list with one label array per recording, each numbered by first appearance within
    its recording and equal to `ahc_cosine_rows` on that recording's rows alone (the scores are the same bits: include/sd_hip_ahc.h).

    A cluster never looks outside its recording, so one nearest pass (`operator.nearest_grouped`, `sd_ahc_nearest_grouped_f32`), one
    merge and one host synchronisation per round serve all recordings: the rounds are the maximum over the recordings, not the sum.
    `group`, the recording of every active cluster, is compacted with the sums and stays non-decreasing because compaction keeps
    order; max(sizes) bounds a recording's clusters in every round, since clusters only merge.  The kernel's verdict on those two
    promises (`bad`) comes back in the same host read as the number of merges; non-zero raises RuntimeError.

    info = {"rounds": rounds that merged something, "clusters": per recording, "gram_tiles": the 128 x 128 tiles computed, summed over
    every nearest pass}.  A non-finite row raises ValueError before anything is launched.

    `min_clusters` / `max_clusters`: a scalar or one value per recording (both None: the threshold cut above, unchanged), as for
    `ahc_cosine_rows`; every recording's count is clamped into its own bounds, all of them by one launch of the cut.  info then also
    has "threshold_clusters" per recording (the count the threshold leaves) and "rounds_full" (the rounds past the threshold)."""
    sizes = [int(s) for s in sizes]
    info = {"rounds": 0, "clusters": [min(s, 1) for s in sizes], "gram_tiles": 0}
    bounds = _bounds(min_clusters, max_clusters, len(sizes))
    operator = operator_for(X, operator, DeviceSums)
    X = torch.as_tensor(X)
    if X.dim() != 2:
        raise ValueError(f"rows must be a matrix [N, D], got {tuple(X.shape)}")
    N = X.shape[0]
    if min(sizes, default=0) < 0 or sum(sizes) != N:
        raise ValueError(f"sizes {sizes} do not add up to the {N} rows")
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    max_group = max(sizes, default=0)
    if max_group <= 1:                                                                  # nothing to merge anywhere
        labels = [np.zeros(s, dtype=int) for s in sizes]
        return (labels, info) if return_info else labels
    if X.shape[1] == 0 or not bool(torch.isfinite(X).all()):
        raise ValueError("rows must be finite and have at least one column")
    dev = operator.device
    sums = operator.normalise(X.to(dev).float())
    if bounds is not None:
        labels = _bounded(operator, sums, sizes, cos_thr, bounds, True, info, want_tiles=return_info)
        return (labels, info) if return_info else labels
    count = torch.ones((N,), dtype=torch.float32, device=dev)
    inv_count = torch.ones((N,), dtype=torch.float32, device=dev)
    group = torch.from_numpy(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)).to(dev)
    cluster_of = torch.arange(N, device=dev)
    tiles = torch.zeros((), dtype=torch.long, device=dev)
    n = N
    while True:
        nn, best, bad = operator.nearest_grouped(sums, inv_count, group, max_group)
        if return_info:
            tiles = tiles + _band_tiles(group, max_group)
        target, n_merged = operator.merge(sums, count, inv_count, nn, best, float(cos_thr))
        m, broken = torch.cat((n_merged.reshape(1), bad.reshape(1))).tolist()           # the host synchronisation of the round
        if broken:
            raise RuntimeError(f"grouped nearest pass over {n} clusters: `group` decreases or a group exceeds max_group={max_group}")
        if m == 0:
            break
        info["rounds"] += 1
        # the compaction of ahc_cosine_rows, with the group of every kept cluster
        target = target.long()
        ids = torch.arange(n, device=dev)
        keep = target == ids
        new_id = torch.cumsum(keep, 0) - 1
        cluster_of = new_id[target[cluster_of]]
        src = torch.empty((n - m + 1,), dtype=torch.long, device=dev)
        src.scatter_(0, torch.where(keep, new_id, torch.full_like(new_id, n - m)), ids)
        src = src[: n - m]
        sums, count, inv_count, group = sums[src], count[src], inv_count[src], group[src]
        n -= m
    flat = cluster_of.cpu().numpy().astype(int)
    labels = [flat[a:b] - (flat[a] if b > a else 0) for a, b in zip(offsets[:-1], offsets[1:])]
    for lab in labels:                                                                  # a recording's cluster ids are a run of the global ones
        assert lab.size == 0 or (lab[0] == 0 and np.all(np.diff(np.maximum.accumulate(lab)) <= 1)), "cluster ids are not numbered by first appearance"
    info["clusters"] = [int(lab.max()) + 1 if lab.size else 0 for lab in labels]
    info["gram_tiles"] = int(tiles)
    return (labels, info) if return_info else labels


class AhcGpuClusterer:
    """`cluster.AhcClusterer` on the device route, for the `clusterer_factory=` argument of `cluster.cluster_hdbscan_two_stage` and
    `diar_diag.cluster_embeddings`: `fit_predict` takes L2-normalised rows (metric "euclidean") and cuts at cosine `cos_thr`, the
    cluster count clamped into [min_clusters, max_clusters] when either is given.  A "precomputed" distance matrix raises ValueError:
    the route needs the rows, not a matrix."""

    def __init__(self, cos_thr: float = 0.70, metric: str = "euclidean", operator=None, min_clusters=None, max_clusters=None, **_ignored):
        if metric != "euclidean":
            raise ValueError(f"AhcGpuClusterer clusters rows (metric='euclidean'); metric={metric!r} has no rows to work on")
        _bounds(min_clusters, max_clusters, 1)
        self.cos_thr = float(cos_thr)
        self.metric = metric
        self.operator = operator
        self.min_clusters, self.max_clusters = min_clusters, max_clusters

    @classmethod
    def factory(cls, cos_thr: float = 0.70, operator=None, min_clusters=None, max_clusters=None):
        return lambda **kw: cls(cos_thr, metric=kw.get("metric", "euclidean"), operator=operator, min_clusters=min_clusters,
                                max_clusters=max_clusters)

    def fit_predict(self, X) -> np.ndarray:
        X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
        if self.operator is None:
            X = upload_rows(X, "AhcGpuClusterer runs on the HIP path (a visible GPU); there is no CPU fallback")
        return ahc_cosine_rows(X, self.cos_thr, operator=self.operator, min_clusters=self.min_clusters, max_clusters=self.max_clusters)
