"""Shared by tests/test_hdbscan_rules.py (CPU) and tests/test_gpu_hdbscan.py: a numpy stand-in for the device operator of
`hdbscan_gpu` (f32 unit rows and an f32 Gram made exactly symmetric, the property the kernels are specified to have), the numpy
statement of the two entries of include/sd_hip_hdbscan.h, an f64 Prim spanning tree of the dense mutual-reachability matrix, the
host clusterings the device route is held to, and the planted inputs both files cluster."""
import numpy as np
import torch

# (min_cluster_size, min_samples, allow_single_cluster): diarize()'s two-stage glue, diar_diag's clusterer, and two more
SETTINGS = [(2, None, True), (6, 3, False), (5, None, True), (15, 5, True)]
# (n, k, noise, outliers) of planted()
SHAPES = [(300, 4, 0.6, 0), (1000, 8, 0.8, 20), (2000, 6, 1.0, 50), (700, 3, 0.5, 0)]
# The input on record for a tie: planted(1000, 8, 0.8, seed 2, 20 outliers).  Its row 2 (an outlier) hangs on the tree by TWO edges,
# (2, 180) and (2, 496), and for min_samples >= 3 both weigh exactly core[2], in float64 as in f32 (test_hdbscan_rules.py asserts it):
# two sub-trees join through the row at one and the same height, and which of them it joins first is decided by the order in which
# scikit-learn's unstable argsort hands the two equal edges to its linkage routine, i.e. by the edge order of whoever built the tree.
# At (6, 3, False) the host and the route disagree on that one point under both metrics, at (5, None, True) and (15, 5, True) under
# "cosine" only; no other row and no other of the 48 combinations of SHAPES x SETTINGS x seeds 0 .. 2 differs.  The input is in no
# label table, at any setting.
RECORDED_NEAR_TIE = ((1000, 8, 0.8, 20), (6, 3, False), 2)
TIED_INPUT = ((1000, 8, 0.8, 20), 2)
# the label table: shape s at seed t takes setting (s + t) % 4, and at seed 0 also setting (s + 3) % 4: every setting at every n.  The
# tied input's turn goes to seed 1 of the same shape.  16 cases.
LABEL_CASES = [(shape, SETTINGS[(si + seed) % 4], seed if (shape, seed) != TIED_INPUT else 1) for si, shape in enumerate(SHAPES)
               for seed in range(3)]
LABEL_CASES += [(shape, SETTINGS[(si + 3) % 4], 0) for si, shape in enumerate(SHAPES)]
assert not [c for c in LABEL_CASES if (c[0], c[2]) == TIED_INPUT] and len(set(LABEL_CASES)) == 16


def planted(n, k, noise, seed, outliers, d=192):
    """k unit centres, n rows around them, the first `outliers` rows replaced by isotropic ones; f32 rows scaled by 1 / (norm + 1e-8)."""
    r = np.random.default_rng(seed)
    C = r.standard_normal((k, d))
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    lab = r.integers(0, k, n)
    X = C[lab] + noise * r.standard_normal((n, d)) / np.sqrt(d)
    X[:outliers] = r.standard_normal((outliers, d))
    X = X.astype(np.float32)
    return X / (np.linalg.norm(X, axis=1, keepdims=True) + 1e-8)


def unit_rows(X):
    """f32 unit rows, a zero row left zero (sklearn `normalize`)."""
    X = np.asarray(X, dtype=np.float32)
    nrm = np.sqrt((X.astype(np.float64) ** 2).sum(1, keepdims=True))
    return (X / np.where(nrm > 0, nrm, 1.0)).astype(np.float32)


# ------------------------------------------------------------------ the two entries, stated in numpy

def gram_f32(rows):
    """The f32 Gram, exactly symmetric (BLAS does not promise a symmetric product; the entries' scores are symmetric)."""
    R = np.asarray(rows, dtype=np.float32)
    G = R @ R.T
    return np.maximum(G, G.T)


def core_from_gram(G, k):
    """The k-th largest off-diagonal entry of every row, duplicates counted."""
    n = G.shape[0]
    S = np.array(G, copy=True)
    S[np.arange(n), np.arange(n)] = -np.inf
    return np.sort(S, axis=1)[:, n - k]


def outgoing_from_gram(G, core, comp):
    """w = min(core_i, core_j, G); per row the maximum over the columns of another component and the lowest column attaining it;
    (-1, -inf) where there is none."""
    core = np.asarray(core)
    comp = np.asarray(comp)
    W = np.minimum(np.minimum(core[:, None], core[None, :]), G).astype(G.dtype)
    W[comp[:, None] == comp[None, :]] = -np.inf
    nn = W.argmax(1).astype(np.int32)
    best = W[np.arange(G.shape[0]), nn]
    nn[best == -np.inf] = -1
    return nn, best


class NumpyRows:
    """`hdbscan_gpu.DeviceRows`' interface over CPU torch tensors; the Gram of the rows is formed once."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.passes = 0
        self._gram = None

    def normalise(self, X):
        return torch.from_numpy(unit_rows(X.numpy()))

    def _G(self, rows):
        if self._gram is None or self._gram[0] is not rows:
            self._gram = (rows, gram_f32(rows.numpy()))
        return self._gram[1]

    def core(self, rows, k):
        self.passes += 1
        return torch.from_numpy(core_from_gram(self._G(rows), k).astype(np.float32))

    def outgoing(self, rows, core, comp):
        self.passes += 1
        nn, best = outgoing_from_gram(self._G(rows), core.numpy(), comp.numpy())
        return torch.from_numpy(nn), torch.from_numpy(best.astype(np.float32))


# ------------------------------------------------------------------ f64 reference

def dot_bound(rows, d):
    """[n, n] f64: (d + 4) 2^-23 |a| |b|, the f32 dot-product bound d 2^-24 |a| |b| with 2 x slack (that of ahc_ref.score_bound with
    unit counts)."""
    nrm = np.sqrt((np.asarray(rows, dtype=np.float64) ** 2).sum(1))
    return (d + 4) * 2.0 ** -23 * (nrm[:, None] * nrm[None, :])


def reach_f64(rows, k):
    """(core f64 [n], W f64 [n, n]): the mutual-reachability cosines of the rows in float64, the diagonal at -inf; k = 0: core = +inf."""
    R = np.asarray(rows, dtype=np.float64)
    G = R @ R.T
    G = np.maximum(G, G.T)
    n = G.shape[0]
    core = core_from_gram(G, k) if k else np.full(n, np.inf)
    W = np.minimum(np.minimum(core[:, None], core[None, :]), G)
    W[np.arange(n), np.arange(n)] = -np.inf
    return core, W


def prim_max_tree(W):
    """Prim on a dense symmetric weight matrix -> the n - 1 weights of a MAXIMUM spanning tree, sorted descending.  Own code: scipy's
    sparse minimum_spanning_tree drops zero weights."""
    n = W.shape[0]
    in_tree = np.zeros(n, bool)
    in_tree[0] = True
    key = np.array(W[0], copy=True)
    key[0] = -np.inf
    out = np.empty(n - 1)
    for t in range(n - 1):
        j = int(np.argmax(np.where(in_tree, -np.inf, key)))
        out[t] = key[j]
        in_tree[j] = True
        key = np.maximum(key, W[j])
    return np.sort(out)[::-1]


def is_spanning_tree(lo, hi, n):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    if len(lo) != n - 1 or np.any(lo == hi):
        return False
    return connected_components(coo_matrix((np.ones(n - 1), (lo, hi)), shape=(n, n)), directed=False)[0] == 1


# ------------------------------------------------------------------ the host clusterings

def host_labels(X, setting, metric):
    """scikit-learn's HDBSCAN as the reference's call sites run it: "euclidean" on the rows, or "precomputed" on 1 - cosine."""
    from sklearn.cluster import HDBSCAN
    from sklearn.metrics.pairwise import cosine_similarity
    mcs, ms, single = setting
    clu = HDBSCAN(min_cluster_size=mcs, min_samples=ms, allow_single_cluster=single, metric=metric)
    return clu.fit_predict(X if metric == "euclidean" else 1 - cosine_similarity(X))


def same_clustering(got, want):
    """The same noise set and the same partition of the rest."""
    got, want = np.asarray(got), np.asarray(want)
    if not np.array_equal(got < 0, want < 0):
        return False
    pairs = set(zip(got.tolist(), want.tolist()))
    return len(pairs) == len(set(got.tolist())) == len(set(want.tolist()))


# ------------------------------------------------------------------ exact inputs for the raw entries

def integer_rows(n, d, ld, seed, lo=-3, hi=4):
    """f32 [n][ld] of small integers in columns [0, d), NaN in [d, ld): every product and every partial sum is an integer below 2^24,
    so the f32 scores are exact in any summation order and ties are plentiful."""
    rng = np.random.default_rng(seed)
    S = np.full((n, ld), np.nan, dtype=np.float32)
    S[:, :d] = rng.integers(lo, hi, (n, d)).astype(np.float32)
    return S
