"""The numpy statement of sd_kmeans_grouped_f64 (include/sd_hip_kmeans.h, "THE RESULT"): scikit-learn's `k_means` (greedy k-means++,
Lloyd, n_init restarts, the best one kept) over random numbers that were drawn in advance, with direct squared distances, all f64.
It also returns the MARGINS that make an integer-for-integer comparison with scikit-learn meaningful (each a minimum over every
restart and iteration: an input whose margins are all far above the rounding of an f64 sum has no near-tie, and any correct
evaluation order gives the same labels) and COUNTERS of the branches taken.  The cases of the rule and the GPU tests live here too."""
import math

import numpy as np

EMPTY, NONFINITE, BAD_K, BAD_DRAW, BAD_PROMISE = 1, 2, 4, 8, 16
MAX_K, MAX_DIM, MAX_INIT = 32, 32, 16
U_CENTRES, U_TRIALS = MAX_K - 1, 5                    # the padded shape of the uniform draws of one restart
MARGIN_BAR = 1e-9
MARGINS = ("assign", "prefix", "trial", "shift", "inertia")
COUNTERS = ("strict", "tol", "exhausted", "displaced", "same", "higher")


def trials_of(k):
    return 2 + int(math.log(k))


def sq_dist(X, C):
    """|X_i - C_c|^2 as [n, k], the differences squared and summed directly"""
    return ((X[:, None, :] - C[None, :, :]) ** 2).sum(axis=2)


def _gap(lo, hi):
    """relative gap of two non-negative numbers lo <= hi"""
    return np.inf if hi <= 0 else (hi - lo) / hi


class Trace:
    def __init__(self):
        self.margins = {m: np.inf for m in MARGINS}
        self.counters = {c: 0 for c in COUNTERS}
        self.iterations = []

    def margin(self, name, value):
        self.margins[name] = min(self.margins[name], float(value))

    def merge(self, other):
        for m in MARGINS:
            self.margin(m, other.margins[m])
        for c in COUNTERS:
            self.counters[c] += other.counters[c]
        self.iterations += other.iterations


def _assign(X, C, tr):
    D = sq_dist(X, C)
    lab = D.argmin(axis=1)
    if D.shape[1] > 1:
        two = np.partition(D, 1, axis=1)[:, :2]
        tr.margin("assign", np.min(np.where(two[:, 1] > 0, (two[:, 1] - two[:, 0]) / np.where(two[:, 1] > 0, two[:, 1], 1), np.inf)))
    return lab.astype(np.int32), D[np.arange(len(X)), lab]


def seed(X, k, first, u, tr):
    """greedy k-means++ from the first centre X[first] and the uniform numbers u[c - 1][j] -> the k centres' rows"""
    n, t = len(X), trials_of(k)
    idx = [int(first)]
    closest = sq_dist(X, X[idx])[:, 0]
    pot = closest.sum()
    for c in range(1, k):
        v = u[c - 1, :t] * pot
        cum = np.cumsum(closest)
        cand = np.minimum(np.searchsorted(cum, v, side="left"), n - 1)
        if pot > 0:
            tr.margin("prefix", np.abs(cum[None, :] - v[:, None]).min() / pot)
        D = np.minimum(closest[None, :], sq_dist(X, X[cand]).T)          # [t, n]
        pots = D.sum(axis=1)
        best = int(np.argmin(pots))
        others = pots[cand != cand[best]]
        if len(others):
            tr.margin("trial", _gap(pots[best], others.min()))
        idx.append(int(cand[best]))
        closest, pot = D[best], pots[best]
    return np.array(idx)


def lloyd(X, C, max_iter, tol, tr):
    """-> (labels, inertia, iterations, empty)"""
    n, k = len(X), len(C)
    old = np.full(n, -1, np.int32)
    strict = False
    it = 0
    for it in range(1, max_iter + 1):
        lab, _ = _assign(X, C, tr)
        count = np.bincount(lab, minlength=k)
        if (count == 0).any():
            return lab, np.nan, it, True
        new = np.zeros_like(C)
        np.add.at(new, lab, X)
        new /= count[:, None]
        shift = ((new - C) ** 2).sum()
        C = new
        if np.array_equal(lab, old):
            strict = True
            tr.counters["strict"] += 1
            break
        if tol > 0:
            tr.margin("shift", abs(shift - tol) / tol)
        if shift <= tol:
            tr.counters["tol"] += 1
            break
        old = lab
    else:
        tr.counters["exhausted"] += 1
    if not strict:
        lab, _ = _assign(X, C, tr)
    inertia = ((X - C[lab]) ** 2).sum(axis=1).sum()
    return lab, inertia, it, False


def same_clustering(a, b, k):
    """scikit-learn's _is_same_clustering"""
    mapping = np.full(k, -1, np.int64)
    for x, y in zip(a, b):
        if mapping[x] == -1:
            mapping[x] = y
        elif mapping[x] != y:
            return False
    return True


def kmeans_one(rows, k, first, u, max_iter=300, tol_rel=1e-4):
    """One recording: rows f64 [n, dim], first int [R], u f64 [R, >= k - 1, >= t] -> dict(labels, chosen, inertia, iters, flags, trace)"""
    rows = np.asarray(rows, np.float64)
    n = len(rows)
    tr = Trace()
    out = dict(labels=np.full(n, -1, np.int32), chosen=-1, inertia=0.0, iters=0, flags=0, trace=tr)
    if not (2 <= k <= MAX_K and k < n):
        out["flags"] = BAD_K
        return out
    if ((np.asarray(first) < 0) | (np.asarray(first) >= n)).any():
        out["flags"] = BAD_DRAW
        return out
    if not np.isfinite(rows).all():
        out["flags"] = NONFINITE
        return out
    X = rows - rows.mean(axis=0)
    tol = tol_rel * np.mean(np.var(X, axis=0)) if tol_rel != 0 else 0.0
    best = None
    for r in range(len(first)):
        C = X[seed(X, k, first[r], u[r], tr)]
        lab, inertia, it, empty = lloyd(X, C, max_iter, tol, tr)
        tr.iterations.append(it)
        if empty:
            out["flags"] = EMPTY
            return out
        if best is None:
            best = (lab, inertia, it, r)
            continue
        same = same_clustering(lab, best[0], k)
        if not same:
            tr.margin("inertia", abs(inertia - best[1]) / max(inertia, best[1]) if max(inertia, best[1]) > 0 else np.inf)
        if inertia < best[1] and not same:
            tr.counters["displaced"] += 1
            best = (lab, inertia, it, r)
        elif inertia < best[1]:
            tr.counters["same"] += 1
        else:
            tr.counters["higher"] += 1
    out.update(labels=best[0], inertia=float(best[1]), iters=best[2], chosen=best[3])
    return out


def promise_holds(first_row, n_rows):
    fr = np.asarray(first_row, np.int64)
    return fr[0] == 0 and fr[-1] == n_rows and (np.diff(fr) >= 0).all()


class NumpyLaunch:
    """The injectable `launch` of kmeans_gpu.k_means_groups, as the statement: same arguments, same five arrays back.  `trace` holds the
    merged margins and counters of every recording of the last call."""

    def __init__(self):
        self.calls = 0
        self.trace = Trace()

    def __call__(self, X, first_row, ks, first, u, n_init, max_iter, tol_rel):
        self.calls += 1
        X = np.asarray(X, np.float64)
        G = len(ks)
        labels = np.full(len(X), -1, np.int32)
        chosen, iters, flags = np.full(G, -1, np.int32), np.zeros(G, np.int32), np.zeros(G, np.int32)
        inertia = np.zeros(G)
        if not promise_holds(first_row, len(X)):
            flags[:] = BAD_PROMISE
            return labels, chosen, inertia, iters, flags
        for g in range(G):
            a, b = int(first_row[g]), int(first_row[g + 1])
            one = kmeans_one(X[a:b], int(ks[g]), np.asarray(first[g][:n_init]), np.asarray(u[g][:n_init]), max_iter, tol_rel)
            labels[a:b], chosen[g], inertia[g], iters[g], flags[g] = one["labels"], one["chosen"], one["inertia"], one["iters"], one["flags"]
            self.trace.merge(one["trace"])
        return labels, chosen, inertia, iters, flags


# ------------------------------------------------------------------ the cases

# (n, d, k, spread, seed)
BLOBS = [(65, 2, 3, 1.0, 0), (257, 5, 4, 1.5, 1), (1000, 8, 8, 2.0, 2), (3001, 16, 12, 2.5, 3), (1000, 32, 32, 3.0, 4), (513, 3, 7, 0.8, 5),
         (2272, 8, 5, 1.0, 6), (129, 2, 16, 1.0, 7), (64, 1, 2, 1.0, 8), (255, 4, 6, 0.5, 9), (1023, 6, 3, 0.3, 10), (700, 12, 10, 1.2, 11)]
PLANTED = [(40, 2), (65, 3), (257, 4), (500, 5), (1000, 8), (300, 12), (33, 32)]


def blob(n, d, k, spread, seed):
    rng = np.random.default_rng(seed)
    C = rng.standard_normal((k, d)) * spread
    lab = rng.integers(0, k, n)
    return C[lab] + rng.standard_normal((n, d))


def degenerate_rows():
    """40 rows of 3 distinct values: k = 5 must leave a cluster empty"""
    return np.repeat(np.array([[0.0, 0.0], [5.0, 1.0], [-3.0, 4.0]]), [14, 13, 13], axis=0)


def sklearn_labels(X, k, random_state, **kw):
    from sklearn.cluster import k_means
    kw.setdefault("n_init", 10)
    centres, labels, inertia, iters = k_means(np.array(X, np.float64), k, random_state=random_state, return_n_iter=True, **kw)
    return labels.astype(np.int32), float(inertia), int(iters)


# ------------------------------------------------------------------ the recordings of the GPU launches

GPU_SIZES = (3, 63, 64, 65, 255, 256, 257, 1000)       # both sides of a wave (64) and of the workgroup (256)
GPU_DIMS = (1, 2, 8, 31, 32)
GPU_KS = (2, 3, 8, 21, 32)
STREAMED = {1: 21000, 2: 10500, 8: 2600, 31: 700, 32: 700}     # n d 8 bytes > 160 KB: these rows cannot live in LDS


# (rows, k, seed) per launch.  k rotates through GPU_KS, held to k < n and, above 3, to at most n / 12 (with a dozen clusters over 63
# rows two candidates of a seeding step often lower the potential by exactly the same amount: a tie that only the summation order
# decides); the seeds are the first of 100 d + i + 1000 a, a = 0, 1, ..., at which every margin is at least 1e-8 (the margin condition
# of the rule tests, which check it again): most are a = 0, the three rows need another because their two candidates often tie exactly.
GPU_CASES = {
    1: [(3, 2, 1100), (63, 3, 101), (64, 3, 102), (65, 3, 103), (255, 21, 104), (256, 2, 105), (257, 3, 106), (1000, 8, 107), (21000, 21, 108)],
    2: [(3, 2, 20200), (63, 3, 201), (64, 3, 202), (65, 3, 203), (255, 2, 204), (256, 3, 205), (257, 8, 206), (1000, 21, 207), (10500, 32, 208)],
    8: [(3, 2, 11800), (63, 3, 801), (64, 3, 802), (65, 2, 803), (255, 3, 804), (256, 8, 805), (257, 21, 806), (1000, 32, 807), (2600, 2, 808)],
    31: [(3, 2, 4100), (63, 3, 3101), (64, 2, 3102), (65, 3, 3103), (255, 8, 3104), (256, 21, 3105), (257, 21, 3106), (1000, 2, 3107),
         (700, 3, 3108)],
    32: [(3, 2, 3200), (63, 2, 3201), (64, 3, 3202), (65, 3, 3203), (255, 21, 3204), (256, 21, 3205), (257, 2, 3206), (1000, 3, 3207),
         (700, 8, 3208)],
}


def gpu_cases(d):
    """The recordings of one launch at `d` columns: every critical size and a streamed one -> [(rows, k, seed)]"""
    assert [n for n, _, _ in GPU_CASES[d]] == list(GPU_SIZES) + [STREAMED[d]] and STREAMED[d] * d * 8 > 160 * 1024
    return [(blob(n, d, k, 4.0, seed), k, seed) for n, k, seed in GPU_CASES[d]]


def reference(cases, **kw):
    """scikit-learn's answer for every recording, and the statement's margins and flags for the same draws (a condition on the
    inputs) -> ([(labels, inertia, iterations)], Trace, flags)"""
    import warnings
    want, launch, flags = [], NumpyLaunch(), []
    n_init = kw.get("n_init", 10)
    for X, k, seed in cases:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want.append(sklearn_labels(X, k, np.random.RandomState(seed), **kw))
        first, uu = draws_padded(np.random.RandomState(seed), len(X), k, n_init)
        out = launch(X, np.array([0, len(X)]), [k], first[None], uu[None], n_init, kw.get("max_iter", 300), kw.get("tol", 1e-4))
        flags.append(int(out[4][0]))
    return want, launch.trace, flags


def draws_padded(rs, n, k, n_init):
    """kmeans_gpu.kmeans_draws in the padded shape of the entry: first int32 [n_init], u f64 [n_init, 31, 5]"""
    from speech_diarization_amd import kmeans_gpu
    first, uu = kmeans_gpu.kmeans_draws(rs, n, k, n_init)
    u = np.zeros((n_init, U_CENTRES, U_TRIALS))
    u[:, :uu.shape[1], :uu.shape[2]] = uu
    return first, u
