"""Shared by tests/test_ahc_rules.py (CPU) and tests/test_gpu_ahc.py: a numpy stand-in for the device operator of `ahc_gpu` (f32 sums
and f32 products, the arithmetic the kernels are specified to do, in numpy's summation order), the f64 reference of the two entries of
include/sd_hip_ahc.h, the cut margin of the host dendrogram, and the inputs both files cluster."""
import numpy as np
import torch

import spectral_ref as R

# (N, planted speakers, noise, seed) of tests/test_spectral_rules.py FAMILIES by row count, and the (rows, cos_thr) pairs the driver is
# held to the host route on: no merge height of the host dendrogram lies within CUT_MARGIN of the cut in any of them.
FAMILY = {400: (400, 2, 0.9, 0), 700: (700, 3, 1.5, 0), 1000: (1000, 4, 2.0, 0), 1300: (1300, 5, 2.5, 1), 1600: (1600, 6, 3.0, 0),
          2000: (2000, 8, 1.2, 0)}
DRIVER_PAIRS = [(400, 0.3), (400, 0.1), (400, 0.0), (700, 0.1), (700, 0.0), (1000, 0.0), (1300, 0.0), (1600, 0.0), (2000, 0.1), (2000, 0.0)]
CUT_MARGIN = 1e-3


def family_rows(rows):
    X, planted = R.planted_rows(*FAMILY[rows])
    return X.astype(np.float32), planted


def duplicates_and_zero_rows():
    """The first 300 rows of the 400-row family, their first 50 again, and 3 zero rows."""
    X, _ = family_rows(400)
    return np.concatenate([X[:300], X[:50], np.zeros((3, X.shape[1]), np.float32)])


def unit_rows(X):
    """f32 unit rows, a zero row left zero (sklearn `normalize`)."""
    X = np.asarray(X, dtype=np.float32)
    nrm = np.sqrt((X.astype(np.float64) ** 2).sum(1, keepdims=True))
    return (X / np.where(nrm > 0, nrm, 1.0)).astype(np.float32)


def host_affinity(X):
    """What the host route clusters: the f32 cosine matrix of the rows (sklearn `cosine_similarity` semantics)."""
    Xn = unit_rows(X)
    return Xn @ Xn.T


# ------------------------------------------------------------------ the two entries, stated in numpy

def nearest_f32(sums, inv_count):
    """score = (S S^T) * (inv inv^T) in f32, the diagonal excluded -> (nn int32, best f32); n == 1: (-1, -inf)."""
    S = np.asarray(sums, dtype=np.float32)
    inv = np.asarray(inv_count, dtype=np.float32)
    n = S.shape[0]
    if n == 1:
        return np.array([-1], np.int32), np.array([-np.inf], np.float32)
    score = (S @ S.T) * (inv[:, None] * inv[None, :])
    score = np.maximum(score, score.T)          # BLAS does not promise a symmetric product; the entry's scores are symmetric
    np.fill_diagonal(score, -np.inf)
    nn = score.argmax(1).astype(np.int32)
    return nn, score[np.arange(n), nn].astype(np.float32)


def merge_f32(sums, count, inv_count, nn, best, cos_thr):
    """The statement of sd_ahc_merge_f32 on copies -> (sums, count, inv_count, target int32, n_merged)."""
    sums, count, inv_count = (np.array(a, dtype=np.float32, copy=True) for a in (sums, count, inv_count))
    n = sums.shape[0]
    target = np.arange(n, dtype=np.int32)
    merged = 0
    for i in range(n):
        j = int(nn[i])
        if i < j < n and int(nn[j]) == i and best[i] > np.float32(cos_thr):
            sums[i] = sums[i] + sums[j]
            count[i] = count[i] + count[j]
            inv_count[i] = np.float32(1.0) / count[i]
            target[j] = i
            merged += 1
    return sums, count, inv_count, target, merged


class NumpySums:
    """`ahc_gpu.DeviceSums`' interface over CPU torch tensors."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.passes = 0

    def normalise(self, X):
        return torch.from_numpy(unit_rows(X.numpy()))

    def nearest(self, sums, inv_count):
        self.passes += 1
        nn, best = nearest_f32(sums.numpy(), inv_count.numpy())
        return torch.from_numpy(nn), torch.from_numpy(best)

    def merge(self, sums, count, inv_count, nn, best, cos_thr):
        s, c, ic, target, merged = merge_f32(sums.numpy(), count.numpy(), inv_count.numpy(), nn.numpy(), best.numpy(), cos_thr)
        sums.copy_(torch.from_numpy(s))
        count.copy_(torch.from_numpy(c))
        inv_count.copy_(torch.from_numpy(ic))
        return torch.from_numpy(target), torch.tensor([merged], dtype=torch.int32)


# ------------------------------------------------------------------ f64 reference of the nearest entry

def score_bound(sums, inv_count, d):
    """[n, n] f64: (d + 4) 2^-23 (|a| |b|) inv_i inv_j, the f32 dot-product bound d 2^-24 |a| |b| (plus the three roundings of the
    scale) with 2 x slack."""
    S = np.asarray(sums, dtype=np.float64)
    inv = np.asarray(inv_count, dtype=np.float64)
    nrm = np.sqrt((S * S).sum(1))
    return (d + 4) * 2.0 ** -23 * (nrm[:, None] * nrm[None, :]) * (inv[:, None] * inv[None, :])


def scores_f64(sums, inv_count):
    """[n, n] f64 scores, the diagonal at -inf."""
    S = np.asarray(sums, dtype=np.float64)
    inv = np.asarray(inv_count, dtype=np.float64)
    score = (S @ S.T) * (inv[:, None] * inv[None, :])
    np.fill_diagonal(score, -np.inf)
    return score


def check_nearest(nn, best, sums, inv_count, d):
    """Assert the contract of sd_ahc_nearest_f32 against f64 -> the largest |best - best64| / bound seen."""
    n = sums.shape[0]
    nn, best = np.asarray(nn), np.asarray(best, dtype=np.float64)
    if n == 1:
        assert nn[0] == -1 and best[0] == -np.inf
        return 0.0
    score = scores_f64(sums, inv_count)
    bound = score_bound(sums, inv_count, d)
    rows = np.arange(n)
    assert np.all((nn >= 0) & (nn < n) & (nn != rows)), "nn outside [0, n) or on the diagonal"
    ref_nn = score.argmax(1)
    ref_best = score[rows, ref_nn]
    b_ref = bound[rows, ref_nn]
    # the score bar: within the bound of the f64 maximum (and the reported score is the chosen column's own score)
    err = np.abs(best - ref_best)
    assert np.all(err <= b_ref), f"best is {np.max(err / np.where(b_ref > 0, b_ref, 1)):.3f} bounds from the f64 maximum"
    assert np.all(np.abs(best - score[rows, nn]) <= bound[rows, nn]), "best is not the score of column nn"
    # the index is the f64 argmax wherever the f64 top two are further apart than twice the bound; elsewhere its f64 score lies
    # within the bound of the maximum
    top2 = np.partition(score, -2, axis=1)[:, -2] if n > 2 else np.full(n, -np.inf)
    clear = ref_best - top2 > 2.0 * b_ref
    assert np.array_equal(nn[clear], ref_nn[clear]), f"{int((nn[clear] != ref_nn[clear]).sum())} clear maxima missed"
    assert np.all(ref_best - score[rows, nn] <= b_ref), "nn is further than the bound below the f64 maximum"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b_ref > 0, err / b_ref, 0.0)
    return float(ratio.max())


def grid_case(n, d, ld, seed):
    """sums f32 [n][ld] with NaN in columns [d, ld), counts a mix of 1 .. 5000 (f32), their f32 reciprocals.  Sums look like cluster
    sums: a random direction of about the count's length."""
    rng = np.random.default_rng(seed)
    count = rng.choice(np.array([1, 1, 2, 3, 7, 50, 333, 5000]), n).astype(np.float32)
    S = np.full((n, ld), np.nan, dtype=np.float32)
    S[:, :d] = (rng.standard_normal((n, d)) / np.sqrt(d) * count[:, None] * rng.uniform(0.5, 1.0, (n, 1))).astype(np.float32)
    return S, count, (np.float32(1.0) / count).astype(np.float32)


# ------------------------------------------------------------------ the host dendrogram

def cut_margin(K, cos_thr):
    """min |h - (1 - cos_thr)| over the merge heights h of scipy's average linkage on the distance matrix `cluster.ahc_cosine` builds
    from K."""
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    D = 1.0 - np.asarray(K, dtype=np.float64)
    D = 0.5 * (D + D.T)
    np.fill_diagonal(D, 0.0)
    np.clip(D, 0.0, None, out=D)
    h = linkage(squareform(D, checks=False), "average")[:, 2]
    return float(np.abs(h - (1.0 - cos_thr)).min())
