"""Shared by tests/test_ahc_cut_rules.py (CPU) and tests/test_gpu_ahc_cut.py: the numpy statement of `sd_ahc_cut_grouped`
(include/sd_hip_cut.h), a numpy operator with `cut` for the bounded drivers of `ahc_gpu`, the scipy oracle of a bounded cut, the
synthetic merge logs both files cut, and the recordings of the driver tests."""
import numpy as np
import torch

import ahc_grouped_ref as AG
import ahc_ref as A

I32_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------ the entry, stated in numpy

def merges_to_apply(n, L, key, cos_thr, lo_bound, hi_bound):
    """m of the header: max(0, min(max(c, n - max), n - min)), c the keys above cos_thr (strict)."""
    c = int((np.asarray(key, np.float32) > np.float32(cos_thr)).sum())
    return max(0, min(max(c, n - int(hi_bound)), n - int(lo_bound)))


def cut_one(lo, hi, key, n, cos_thr, lo_bound, hi_bound):
    """One recording of n rows -> (labels int32 [n], clusters, bad).  A bad recording: labels -1, clusters 0."""
    lo, hi, key = np.asarray(lo, np.int64), np.asarray(hi, np.int64), np.asarray(key, np.float32)
    L = len(key)
    refuse = (np.full(n, -1, np.int32), 0, 1)
    if lo_bound < 1 or lo_bound > hi_bound or L > max(n - 1, 0):
        return refuse
    if L and ((lo < 0) | (lo >= hi) | (hi >= n) | ~np.isfinite(key)).any():
        return refuse
    m = merges_to_apply(n, L, key, cos_thr, lo_bound, hi_bound)
    if m > L:
        return refuse
    order = np.lexsort((np.arange(L), -(key + np.float32(0.0)).astype(np.float64)))          # key descending, position ascending; -0.0 is 0.0
    applied = order[:m]
    parent = np.arange(n)
    for i in applied:
        if parent[hi[i]] not in (hi[i], lo[i]):
            return refuse                                                   # a row absorbed twice, into different clusters
        parent[hi[i]] = lo[i]
    root = np.arange(n)
    for p in range(n):                                                      # parent[x] < x for every non-root: ascending order resolves it
        root[p] = p if parent[p] == p else root[parent[p]]
    is_root = parent == np.arange(n)
    rank = np.cumsum(is_root) - 1
    return rank[root].astype(np.int32), n - m, 0


def cut_numpy(lo, hi, key, first_merge, first_row, cos_thr, min_clusters, max_clusters):
    """The entry -> (labels int32 [rows], clusters int32 [G], bad int32 [G])."""
    fm, fr = np.asarray(first_merge, np.int64), np.asarray(first_row, np.int64)
    G = len(fr) - 1
    M, rows = len(key), int(fr[-1]) if len(fr) else 0
    promise = fm[0] == 0 and fr[0] == 0 and fm[-1] == M and (np.diff(fm) >= 0).all() and (np.diff(fr) >= 0).all()
    if not promise:
        rows = max(rows, 0)
        return np.full(rows, -1, np.int32), np.zeros(G, np.int32), np.ones(G, np.int32)
    labels, clusters, bad = np.empty(rows, np.int32), np.empty(G, np.int32), np.empty(G, np.int32)
    for g in range(G):
        a, b, r0, r1 = fm[g], fm[g + 1], fr[g], fr[g + 1]
        labels[r0:r1], clusters[g], bad[g] = cut_one(lo[a:b], hi[a:b], key[a:b], int(r1 - r0), cos_thr, int(min_clusters[g]), int(max_clusters[g]))
    return labels, clusters, bad


class NumpyCutSums(AG.NumpyGroupedSums):
    """`ahc_gpu.DeviceSums`' interface over CPU torch tensors, `cut` included; keeps what `cut` was handed."""

    def __init__(self):
        super().__init__()
        self.cut_calls = 0
        self.seen = None

    def cut(self, lo, hi, key, first_merge, first_row, cos_thr, min_clusters, max_clusters):
        self.cut_calls += 1
        self.seen = tuple(t.numpy().copy() for t in (lo, hi, key, first_merge, first_row, min_clusters, max_clusters))
        labels, clusters, bad = cut_numpy(*self.seen[:5], cos_thr, *self.seen[5:])
        return torch.from_numpy(labels), torch.from_numpy(clusters), torch.from_numpy(bad)


# ------------------------------------------------------------------ the oracle

def relabel(labels):
    """Numbered by first appearance."""
    labels = np.asarray(labels)
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse].astype(int)


def host_linkage(X):
    """scipy's average linkage on the f64 distance matrix `cluster.ahc_cosine` builds from the f32 cosine matrix of the rows."""
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    D = 1.0 - np.asarray(A.host_affinity(X), dtype=np.float64)
    D = 0.5 * (D + D.T)
    np.fill_diagonal(D, 0.0)
    np.clip(D, 0.0, None, out=D)
    return linkage(squareform(D, checks=False), "average")


def threshold_clusters(Z, cos_thr):
    """The clusters the threshold cut of `cluster.ahc_cosine` leaves: merges at a height below 1 - cos_thr are applied."""
    return len(Z) + 1 - int((Z[:, 2] < 1.0 - cos_thr).sum())


def oracle_k(Z, cos_thr, lo_bound, hi_bound):
    n = len(Z) + 1
    return min(max(threshold_clusters(Z, cos_thr), min(lo_bound, n)), min(hi_bound, n))


def oracle_labels(Z, k):
    """`fcluster(Z, k, "maxclust")`, numbered by first appearance."""
    from scipy.cluster.hierarchy import fcluster
    return relabel(fcluster(Z, k, "maxclust"))


def cut_gap(Z, k):
    """The difference between the two merge heights on either side of the cut into k clusters (inf at k = 1 and k = n)."""
    n = len(Z) + 1
    if k <= 1 or k >= n:
        return float("inf")
    return float(Z[n - k, 2] - Z[n - k - 1, 2])          # merge n - k (0-based) is the first one not applied


# ------------------------------------------------------------------ synthetic logs

SIZES = (0, 1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1000, 1)


def random_log(n, seed, full=True, equal_keys=False):
    """A valid log of a recording of n rows: a random sequence of merges of the current clusters (lo, hi: their lowest rows, lo < hi),
    keys descending-ish and then made monotone (a key never exceeds a child's), f32.  `full`: n - 1 merges, else about half.
    `equal_keys`: keys drawn from four values, so parents and children tie and the position decides."""
    rng = np.random.default_rng(1000 * n + seed)
    L = max(n - 1, 0) if full else max(n - 1, 0) // 2
    firsts = list(range(n))
    height = {r: np.float32(np.inf) for r in firsts}
    lo, hi, key = np.zeros(L, np.int32), np.zeros(L, np.int32), np.zeros(L, np.float32)
    for i in range(L):
        x, y = sorted(rng.choice(len(firsts), 2, replace=False).tolist())
        a, b = firsts[x], firsts[y]
        raw = np.float32(rng.choice([0.75, 0.5, 0.25, -0.25])) if equal_keys else np.float32(rng.uniform(-0.5, 1.0))
        k = min(raw, height[a], height[b])
        lo[i], hi[i], key[i] = a, b, k
        height[a] = k
        firsts.pop(y)
    return lo, hi, key


def pack(logs, sizes):
    """[(lo, hi, key)] and the rows of every recording -> (lo, hi, key, first_merge, first_row)."""
    lo = np.concatenate([l[0] for l in logs]).astype(np.int32) if logs else np.zeros(0, np.int32)
    hi = np.concatenate([l[1] for l in logs]).astype(np.int32) if logs else np.zeros(0, np.int32)
    key = np.concatenate([l[2] for l in logs]).astype(np.float32) if logs else np.zeros(0, np.float32)
    first_merge = np.concatenate([[0], np.cumsum([len(l[2]) for l in logs])]).astype(np.int32)
    first_row = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return lo, hi, key, first_merge, first_row


def bounds_cases(sizes, logs, cos_thr):
    """{name: (min_clusters, max_clusters)} per recording: binding at min, binding at max, min == max, and not binding."""
    thr_clusters = [n - int((l[2] > np.float32(cos_thr)).sum()) for n, l in zip(sizes, logs)]
    return {
        "min": (np.array([c + 3 for c in thr_clusters], np.int32), np.full(len(sizes), I32_MAX, np.int32)),
        "max": (np.ones(len(sizes), np.int32), np.array([max(1, c // 2) for c in thr_clusters], np.int32)),
        "equal": (np.array([max(1, min(4, n)) for n in sizes], np.int32), np.array([max(1, min(4, n)) for n in sizes], np.int32)),
        "free": (np.ones(len(sizes), np.int32), np.array([max(1, n) for n in sizes], np.int32)),
    }


# ------------------------------------------------------------------ the drivers' recordings

K_RANGE = range(1, 13)
GAP_BAR = 1e-4          # a (recording, k) is compared only when the heights on both sides of the cut are further apart than this


def log_linkage(lo, hi, key, n):
    """A FULL log (n - 1 merges, keys monotone) as a scipy linkage matrix: the merges in the order (key descending, position ascending),
    which keeps children before parents, at heights 1, 2, ...: `fcluster(Z, k, "maxclust")` is then the oracle of the cut into k."""
    L = len(key)
    assert L == n - 1
    order = np.lexsort((np.arange(L), -np.asarray(key, np.float64)))
    node, size = {r: r for r in range(n)}, {r: 1 for r in range(n)}             # by lowest row: the scipy id and the rows of the cluster
    Z = np.zeros((L, 4))
    for t, i in enumerate(order):
        a, b = int(lo[i]), int(hi[i])
        size[a] += size.pop(b)
        Z[t] = (node[a], node.pop(b), t + 1.0, size[a])
        node[a] = n + t
    return Z


DRIVER_CASES = [(0.3, k, k) for k in K_RANGE] + [(0.3, 2, 6), (0.1, 2, 6), (0.0, 2, 6), (0.3, 4, 6)]       # (cos_thr, min, max)


def driver_recordings():
    """The three families with the tiny recordings between them: `ahc_grouped_ref.driver_recordings` at the threshold that holds all."""
    return AG.driver_recordings(0.0)


_LINKAGE = {}


def family_linkage(family):
    """The host linkage of a family, computed once per session."""
    if family not in _LINKAGE:
        _LINKAGE[family] = host_linkage(A.family_rows(family)[0])
    return _LINKAGE[family]


def check_driver_case(labels, case, recs):
    """The labels of `ahc_cosine_groups(..., min, max)` on `recs` against the oracle -> the (family, k) pairs left out for their gap."""
    thr, lo_bound, hi_bound = case
    skipped = []
    for (family, x), got in zip(recs, labels):
        n = len(x)
        if family is None:                                                  # 2 rows at cosine 0.6, none, one
            want = [0, 1] if n == 2 and (lo_bound >= 2 or (thr >= 0.6 and hi_bound >= 2)) else [0] * n
            assert got.tolist() == want, (case, n, got)
            continue
        Z = family_linkage(family)
        k = oracle_k(Z, thr, lo_bound, hi_bound)
        if cut_gap(Z, k) < GAP_BAR:
            skipped.append((family, k))
            continue
        want = oracle_labels(Z, k)
        assert int(got.max()) + 1 == k and np.array_equal(got, want), (case, family, k, int(got.max()) + 1, int((got != want).sum()))
    return skipped


def counter_example():
    """Six unit rows A .. F: cos(A, B) = 0.5, cos(A, E) = cos(B, E) = 0.3, cos(C, D) = 0.1, every other pair 0.  The greedy dendrogram
    merges (A, B) at 0.5, then (AB, E) at 0.3, then (C, D) at 0.1; the first ROUND merges (A, B) and (C, D) together."""
    Gm = np.eye(6)
    for i, j, v in ((0, 1, 0.5), (0, 4, 0.3), (1, 4, 0.3), (2, 3, 0.1)):
        Gm[i, j] = Gm[j, i] = v
    return np.linalg.cholesky(Gm).astype(np.float32)
