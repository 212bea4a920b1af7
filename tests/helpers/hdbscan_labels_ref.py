"""Shared by tests/test_hdbscan_labels_rules.py (CPU) and tests/test_gpu_hdbscan_labels.py: the references of the labelling entry of
include/sd_hip_tree.h (`sd_tree_labels_grouped`), the spanning trees both files label, and a numpy operator with `tree_labels`.

THE ORACLE is scikit-learn 1.7.2's `make_single_linkage` and `tree_to_labels` on the STABLY sorted edge list (`oracle_labels`; the one
place of the tests of this entry that imports the private names).  `labels_of_tree_ref` restates the algorithm in plain numpy / Python
from its description (sort, union-find dendrogram, breadth-first condensation, stabilities in condensed-tree order, excess of mass,
labels); the CPU test holds it to the oracle on every case of the GPU list, and it is the "numpy operator" the driver tests run on."""
import numpy as np
import torch

import hdbscan_grouped_ref as HG

# (min_cluster_size, allow_single_cluster)
SETTINGS = [(2, True), (2, False), (6, False), (15, True)]
LDS_ROWS = (160 * 1024 - 256) // 72          # derived as the header derives it: 72 bytes a row, 256 bytes of a CU's 160 KB kept back
SIZES = (17, 64, 129, 500, LDS_ROWS, LDS_ROWS + 1, 2 * LDS_ROWS + 3)
FAMILIES = ("distinct", "four", "zeros")
SEEDS = (0, 1, 2)


# ------------------------------------------------------------------ the oracle

def oracle_labels(lo, hi, dist, min_cluster_size, allow_single_cluster):
    from sklearn.cluster._hdbscan._linkage import MST_edge_dtype, make_single_linkage
    from sklearn.cluster._hdbscan._tree import tree_to_labels
    dist = np.asarray(dist, dtype=np.float64)
    mst = np.empty(len(dist), dtype=MST_edge_dtype)
    mst["current_node"], mst["next_node"], mst["distance"] = lo, hi, dist
    order = np.argsort(dist, kind="stable")
    labels = tree_to_labels(make_single_linkage(mst[order]), int(min_cluster_size), "eom", bool(allow_single_cluster), 0.0, None)[0]
    return np.asarray(labels).astype(np.int32)


# ------------------------------------------------------------------ the algorithm, restated

def is_spanning_tree(lo, hi, n):
    """n - 1 edges with both ends in [0, n) that never join two rows of one component."""
    lo, hi = np.asarray(lo), np.asarray(hi)
    if len(lo) != n - 1 or len(hi) != n - 1 or n < 2 or lo.min() < 0 or hi.min() < 0 or lo.max() >= n or hi.max() >= n:
        return False
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(lo.tolist(), hi.tolist()):
        ra, rb = find(a), find(b)
        if ra == rb:
            return False
        parent[ra] = rb
    return True


def labels_of_tree_ref(lo, hi, dist, min_cluster_size, allow_single_cluster):
    """The labels of the n = len(dist) + 1 rows whose spanning tree is (lo, hi, dist) -> int32 [n]."""
    dist = np.asarray(dist, dtype=np.float64)
    m, n, mcs = len(dist), len(dist) + 1, int(min_cluster_size)
    order = np.argsort(dist, kind="stable")
    lo, hi, dist = np.asarray(lo)[order].tolist(), np.asarray(hi)[order].tolist(), dist[order]
    with np.errstate(divide="ignore", invalid="ignore"):               # inf - inf = NaN is part of the statement
        return _labels_of_sorted_tree(lo, hi, dist, m, n, mcs, bool(allow_single_cluster))


def _labels_of_sorted_tree(lo, hi, dist, m, n, mcs, allow_single_cluster):
    with np.errstate(divide="ignore"):
        lam = np.where(dist > 0.0, 1.0 / np.where(dist > 0.0, dist, 1.0), np.inf)
    # the dendrogram: edge i makes node n + i
    parent = [-1] * (2 * n - 1)

    def find(x):
        r = x
        while parent[r] >= 0:
            r = parent[r]
        while parent[x] >= 0:
            parent[x], x = r, parent[x]
        return r
    left, right, size = [0] * m, [0] * m, [1] * n + [0] * m
    for i in range(m):
        left[i], right[i] = find(lo[i]), find(hi[i])
        assert left[i] != right[i], "not a tree"
        size[n + i] = size[left[i]] + size[right[i]]
        parent[left[i]] = parent[right[i]] = n + i
    # condense breadth-first over the live nodes; cluster ids 0, 1, ... in the order they are made
    cluster_of = {2 * n - 2: 0}
    birth, stab, cparent, children = [0.0], [np.float64(0.0)], [-1], [None]
    fell_cluster, fell_lam = [0] * n, [0.0] * n
    root_lams = []
    queue, head = [2 * n - 2], 0
    while head < len(queue):
        v = queue[head]
        head += 1
        c, lv = cluster_of[v], np.float64(lam[v - n])
        term = lv - np.float64(birth[c])
        if c == 0:
            root_lams.append(lv)
        L, R = left[v - n], right[v - n]
        if size[L] >= mcs and size[R] >= mcs:
            children[c] = len(stab)
            for side in (L, R):
                cluster_of[side] = len(stab)
                birth.append(lv), stab.append(np.float64(0.0)), cparent.append(c), children.append(None)
                stab[c] = stab[c] + term * np.float64(size[side])
                queue.append(side)
            continue
        for side in (L, R):
            if size[side] >= mcs:
                cluster_of[side] = c
                queue.append(side)
                continue
            sub, sh = [side], 0
            while sh < len(sub):
                u = sub[sh]
                sh += 1
                if u < n:
                    fell_cluster[u], fell_lam[u] = c, lv
                    stab[c] = stab[c] + term
                else:
                    sub += [left[u - n], right[u - n]]
    K = len(stab)
    # excess of mass
    selected = [False] * K
    with np.errstate(invalid="ignore"):
        for c in range(K - 1, -1 if allow_single_cluster else 0, -1):
            sub = np.float64(0.0)
            if children[c] is not None:
                sub = sub + stab[children[c]]
                sub = sub + stab[children[c] + 1]
            if sub > stab[c]:
                stab[c] = sub
            else:
                selected[c] = True
    code, covered, n_sel = [-1] * K, [False] * K, 0
    for c in range(K):
        above = covered[cparent[c]] if c else False
        if selected[c] and not above:
            code[c], covered[c] = (-2 if c == 0 else n_sel), True
            n_sel += 1
        else:
            code[c], covered[c] = (code[cparent[c]] if above else -1), above
    thr = max(root_lams)
    out = np.empty(n, dtype=np.int32)
    for p in range(n):
        label = code[fell_cluster[p]]
        out[p] = label if label != -2 else (0 if fell_lam[p] >= thr else -1)
    return out


# ------------------------------------------------------------------ spanning trees

def _distances(m, family, rng):
    if family == "distinct":
        d = rng.random(m) + 0.01
        assert len(np.unique(d)) == m
        return d
    if family == "four":
        return rng.choice(np.array([0.25, 0.5, 0.75, 1.25]), m)
    assert family == "zeros"
    d = rng.random(m) + 0.01
    d[rng.permutation(m)[:max(1, m // 4)]] = 0.0
    return d


def random_tree(n, seed, family="distinct"):
    """Row i > 0 hangs on a random earlier row; then the rows and the edge order are permuted -> (lo int32, hi int32, dist f64)."""
    rng = np.random.default_rng([n, seed, FAMILIES.index(family)])
    a = np.arange(1, n)
    b = (rng.random(n - 1) * a).astype(np.int64)
    rows = rng.permutation(n)
    swap = rng.random(n - 1) < 0.5
    lo, hi = rows[np.where(swap, a, b)], rows[np.where(swap, b, a)]
    order = rng.permutation(n - 1)
    return lo[order].astype(np.int32), hi[order].astype(np.int32), _distances(n - 1, family, rng)[order]


def path_tree(n, seed=0):
    """0 - 1 - ... - n - 1 with growing distances: the deepest dendrogram."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n - 1)
    a = np.arange(n - 1)
    return a[order].astype(np.int32), (a + 1)[order].astype(np.int32), (0.5 + a / n)[order]


def star_tree(n, seed=0):
    """Every row hangs on row 0 at ONE distance: every edge ties, and the dendrogram is a comb in list order."""
    a = np.arange(1, n)
    return np.zeros(n - 1, np.int32), a.astype(np.int32), np.full(n - 1, 0.5)


def balanced_tree(n, seed=0):
    """Row i hangs on row (i - 1) // 2, distances falling with depth: the shallowest dendrogram with many true splits."""
    a = np.arange(1, n)
    return ((a - 1) // 2).astype(np.int32), a.astype(np.int32), 1.0 / (1.0 + np.floor(np.log2(a + 1))) + 1e-6 * a


def small_trees():
    """n = 2, 3 and 5 rows."""
    return [("two", np.array([0], np.int32), np.array([1], np.int32), np.array([0.7])),
            ("three", np.array([2, 0], np.int32), np.array([1, 2], np.int32), np.array([0.9, 0.4])),
            ("three_tied", np.array([0, 1], np.int32), np.array([1, 2], np.int32), np.array([0.5, 0.5])),
            ("five", np.array([3, 0, 4, 1], np.int32), np.array([0, 1, 3, 2], np.int32), np.array([0.3, 0.8, 0.31, 0.2])),
            ("five_zero", np.array([3, 0, 4, 1], np.int32), np.array([0, 1, 3, 2], np.int32), np.array([0.0, 0.8, 0.0, 0.2]))]


def random_cases():
    """[(name, lo, hi, dist)]: every size x family x seed of the lists above, and a path, a star and a balanced tree."""
    out = [(f"{family}{n}s{seed}", *random_tree(n, seed, family)) for n in SIZES for family in FAMILIES for seed in SEEDS]
    for n in (129, LDS_ROWS + 1):
        out += [(f"path{n}", *path_tree(n)), (f"star{n}", *star_tree(n)), (f"balanced{n}", *balanced_tree(n))]
    return out


BREAKAGES = ("cycle", "high", "negative", "nan")


def break_tree(tree, kind):
    """A copy of the tree that is none any more: an edge repeated (a cycle), an index equal to the number of rows, an index of -1, a
    NaN distance."""
    lo, hi, dist = (np.array(x, copy=True) for x in tree)
    if kind == "cycle":
        lo[5], hi[5] = lo[4], hi[4]
    elif kind == "high":
        hi[7] = len(dist) + 1
    elif kind == "negative":
        lo[7] = -1
    else:
        assert kind == "nan"
        dist[3] = np.nan
    return lo, hi, dist


def pack(trees):
    """[(lo, hi, dist)] -> (lo, hi, dist, first_edge int32 [G + 1], max_edges) of one launch."""
    first = np.concatenate([[0], np.cumsum([len(t[2]) for t in trees])]).astype(np.int32)
    lo, hi = (np.concatenate([np.asarray(t[i], dtype=np.int32) for t in trees]) for i in (0, 1))
    dist = np.concatenate([np.asarray(t[2], dtype=np.float64) for t in trees])
    return lo, hi, dist, first, int(np.diff(first).max())


def unpack(labels, first_edge):
    """The label array of one launch -> one array per recording (its rows start at first_edge[g] + g)."""
    first_edge = np.asarray(first_edge)
    return [np.asarray(labels[first_edge[g] + g:first_edge[g + 1] + g + 1]) for g in range(len(first_edge) - 1)]


# ------------------------------------------------------------------ the numpy operator

def tree_labels_numpy(lo, hi, dist, first_edge, max_edges, min_cluster_size, allow_single_cluster):
    """The entry, stated: (labels int32 [n_edges + n_groups], bad int32 [n_groups])."""
    G = len(first_edge) - 1
    labels = np.full(len(dist) + G, -1, dtype=np.int32)
    bad = np.zeros(G, dtype=np.int32)
    for g in range(G):
        a, b = int(first_edge[g]), int(first_edge[g + 1])
        d = dist[a:b]
        ok = 1 <= b - a <= max_edges and np.isfinite(d).all() and (d >= 0).all() and is_spanning_tree(lo[a:b], hi[a:b], b - a + 1)
        bad[g] = 0 if ok else 1
        if ok:
            labels[a + g:b + g + 1] = labels_of_tree_ref(lo[a:b], hi[a:b], d, min_cluster_size, allow_single_cluster)
    return labels, bad


class NumpyLabelRows(HG.NumpyGroupedRows):
    """`hdbscan_gpu.DeviceRows`' interface over CPU torch tensors, `tree_labels` included; `label_calls` counts its calls."""
    label_calls = 0

    def tree_labels(self, lo, hi, dist, first_edge, max_edges, min_cluster_size, allow_single_cluster):
        self.label_calls += 1
        assert lo.dtype == hi.dtype == first_edge.dtype == torch.int32 and dist.dtype == torch.float64
        labels, bad = tree_labels_numpy(lo.numpy(), hi.numpy(), dist.numpy(), first_edge.numpy(), int(max_edges), int(min_cluster_size),
                                        bool(allow_single_cluster))
        return torch.from_numpy(labels), torch.from_numpy(bad)
