"""Shared by tests/test_spectral_rules.py (CPU) and tests/test_gpu_spectral.py: a numpy stand-in for the device operator of
`cluster_gpu` (f32 products, the arithmetic the kernels are specified to do, in numpy's summation order), the f64 reference of the two
entries, and the seeded planted-cluster inputs."""
import numpy as np
import torch


class NumpyOperator:
    """max(sym(K), 0) in f32 with the `degree` / `apply` interface of `cluster_gpu.DeviceOperator`, over CPU torch tensors."""

    def __init__(self, K):
        K = np.asarray(K, dtype=np.float64)
        self.A = np.clip(0.5 * (K + K.T), 0.0, None).astype(np.float32)
        self.A0 = self.A.copy()
        np.fill_diagonal(self.A0, 0.0)
        self.n = self.A.shape[0]
        self.device = torch.device("cpu")
        self.passes = 0

    def degree(self, zero_diag):
        return torch.from_numpy((self.A0 if zero_diag else self.A).sum(1, dtype=np.float32))

    def apply(self, scale, V, zero_diag):
        self.passes += 1
        s = scale.numpy().astype(np.float32)
        A = self.A0 if zero_diag else self.A
        return torch.from_numpy(s[:, None] * (A @ (s[:, None] * V.numpy().astype(np.float32))))


def planted_rows(n, k, noise, seed, dim=192, dtype=np.float64):
    """n centred rows around k planted unit directions (cluster sizes uneven, every cluster present) -> (rows, labels)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((k, dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    labels = np.concatenate([np.arange(k), rng.integers(0, k, n - k)])
    rng.shuffle(labels)
    X = centres[labels] + noise * rng.standard_normal((n, dim)) / np.sqrt(dim)
    X = X - X.mean(0, keepdims=True)
    return X.astype(dtype), labels


def cosine(X):
    Xn = X / np.linalg.norm(X, axis=1, keepdims=True)
    return Xn @ Xn.T


def host_eigengaps(K, min_speakers, max_speakers):
    """The eigenvalues and gaps `cluster.estimate_num_speakers` decides on (its own arithmetic) -> (ev[: hi + 1], candidate gaps)."""
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    lo, hi = max(1, min_speakers), max(1, min(max_speakers, n))
    A = np.clip(0.5 * (K + K.T), 0.0, None)
    d = A.sum(1)
    d[d <= 0] = 1.0
    ev = np.sort(np.linalg.eigvalsh(np.eye(n) - A / np.sqrt(d[:, None] * d[None, :])))[: hi + 1]
    return ev, np.diff(ev)[lo - 1: hi]


def degree_ref(K, zero_diag):
    A = np.clip(np.asarray(K, dtype=np.float64), 0.0, None)
    if zero_diag:
        np.fill_diagonal(A, 0.0)
    return A.sum(1)


def apply_ref(K, scale, V, zero_diag):
    """f64 product and the elementwise magnitude sum (|S| . |V|) the error bound is stated against."""
    A = np.clip(np.asarray(K, dtype=np.float64), 0.0, None)
    if zero_diag:
        np.fill_diagonal(A, 0.0)
    s = np.asarray(scale, dtype=np.float64)
    S = s[:, None] * A * s[None, :]
    V = np.asarray(V, dtype=np.float64)
    return S @ V, S @ np.abs(V)


# ------------------------------------------------------------------ the shape grid of the two entries (tests and tools/spectral_accuracy.py)

GRID_N = (1, 5, 127, 128, 129, 1000, 3001)
GRID_B = (8, 16, 24, 32)


def grid_lds(n):
    """Two row strides > n: an odd one (rows not 16-byte aligned: the scalar loads) and a multiple of 4 (the 16-byte loads)."""
    return (n + 3 if (n + 3) % 4 else n + 5, (n + 3) // 4 * 4 + 4)


def grid_affinity(n, ld, seed):
    """A symmetric [n][ld] f32 affinity in [-1, 1] (about half of it negative), unit diagonal, a few rows without a positive entry
    (diagonal included), NaN in the padding columns [n, ld): a kernel that reads them poisons its result."""
    rng = np.random.default_rng(seed)
    K = rng.uniform(-1.0, 1.0, (n, n))
    K = 0.5 * (K + K.T)
    np.fill_diagonal(K, 1.0)
    for i in sorted(set((n // 3, n - 1)) if n >= 5 else ()):
        K[i, :] = -np.abs(K[i, :])
        K[:, i] = K[i, :]
    out = np.full((n, ld), np.nan, dtype=np.float32)
    out[:, :n] = K.astype(np.float32)
    return out


def grid_scale(K, zero_diag):
    """f32 1 / sqrt(deg) from the f64 degrees, 1 for a zero-degree row."""
    d = degree_ref(K, zero_diag)
    return np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 1.0).astype(np.float32)


def grid_block(n, b, seed):
    return np.random.default_rng(seed + 7919).standard_normal((n, b)).astype(np.float32)


def apply_error_over_bound(Y, K, scale, V, zero_diag):
    """max over elements of |Y - Y64| / (N 2^-23 (|S| |V|)): the share of the worst-case f32 bound an output uses (<= 1 is the
    contract).  Elements whose bound is 0 must be exactly 0 (they count as 0, or as inf when they are not)."""
    n = K.shape[0]
    Y64, mag = apply_ref(K, scale, V, zero_diag)
    err = np.abs(np.asarray(Y, dtype=np.float64) - Y64)
    bound = n * 2.0 ** -23 * mag
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max()) if ratio.size else 0.0
