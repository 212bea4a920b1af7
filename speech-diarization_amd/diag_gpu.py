"""Device route for the whitening and the cluster centres of the reference's "VBx-like" diarizer [REF diar_diag.py:187-194, 373-383].

`cluster.whiten_l2` centres the embeddings, takes the covariance, and multiplies by its inverse square root with a floor of 1e-6 on
the eigenvalues, all in float64.  The floor is why float64 matters: an f32 covariance is wrong by about 1e-7 . lambda_max, above the
floor as soon as lambda_max > 10, and the directions the floor protects are exactly the ones 1 / sqrt blows up.  The two O(N d^2)
parts therefore run in f64 on the f64 matrix cores (include/sd_hip_diag.h), and the d x d part between them stays on the host:

* `stats`: column means and the centred Gram matrix (`ops.whiten_stats`, `sd_whiten_stats_f64`), two passes as `np.cov`;
* the host divides by n - 1, takes `eigh` of the d x d covariance and forms W = U diag(1 / sqrt(max(S, 0) + 1e-6)) U^T in numpy
  f64 (d <= 256: 2 x 512 KB cross the bus, nothing that grows with N);
* `apply`: (x - mean) W in f64, divided by (its norm + 1e-9), rounded to f32 once (`ops.whiten_apply`, `sd_whiten_apply_f64`).
Cluster centres (`centroids`, `ops.label_centroids`, `sd_label_centroids_f32`) are the unit mean of every label's rows, accumulated in
f64 in row order.

The operator is injectable (`operator=`): an object with `device`, `stats(X)`, `apply(X, mean, W)` and `centroids(X, labels, k)` over
torch tensors.  `DeviceDiag` is the product one; the tests run the same driver on the CPU against a numpy operator.  There is no
implicit CPU route: without an operator a host tensor raises the product path's RuntimeError.

One difference from the host route: the result is f32 (one rounding, 2^-25 for an entry <= 1), and the f64 sums are added in the
kernels' order, not numpy's.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .device_rows import DeviceRoute, operator_for

EIG_FLOOR = 1e-6          # [REF diar_diag.py:191]
NORM_EPS = 1e-9           # [REF diar_diag.py:193, 381]


def _f32(X: torch.Tensor) -> torch.Tensor:
    """X as f32 with contiguous rows; `ops.rows4` does the rest (a padded copy where the stride or the alignment demands one)."""
    X = X.float()
    return X if X.stride(1) == 1 else X.contiguous()


class DeviceDiag(DeviceRoute):
    """The three entries of include/sd_hip_diag.h over rows that live on the GPU; the workspace is kept between calls."""
    route = "whitening"

    def stats(self, X: torch.Tensor):
        return ops.whiten_stats(_f32(X), ws=self.ws)

    def apply(self, X: torch.Tensor, mean: torch.Tensor, W: torch.Tensor) -> torch.Tensor:
        return ops.whiten_apply(_f32(X), mean, W, NORM_EPS)

    def centroids(self, X: torch.Tensor, labels: torch.Tensor, k: int):
        return ops.label_centroids(_f32(X), labels.to(torch.int32).contiguous(), k, NORM_EPS)


def _operator(X, operator, what: str):
    operator = operator_for(X, operator, DeviceDiag)
    X = torch.as_tensor(X)
    if X.dim() != 2 or X.shape[1] == 0:
        raise ValueError(f"{what}: rows must be a matrix [N, D >= 1], got {tuple(X.shape)}")
    return X, operator


def whitening_matrix(gram: np.ndarray, n: int) -> np.ndarray:
    """W = U diag(1 / sqrt(max(S, 0) + 1e-6)) U^T of the covariance gram / (n - 1), numpy f64 (the host part of `whiten_l2_rows`;
    the same expression as `cluster.whiten_l2`)."""
    S, U = np.linalg.eigh(np.atleast_2d(np.asarray(gram, dtype=np.float64) / (n - 1)))
    return (U / np.sqrt(np.clip(S, 0.0, None) + EIG_FLOOR)) @ U.T


def whiten_l2_rows(X, *, operator=None) -> torch.Tensor:
    """`cluster.whiten_l2(X)` from rows X f32 [N, D <= 256] on the operator's device -> f32 [N, D], still there.
    N < 2 raises ValueError (np.cov of one row is NaN); a non-finite row raises ValueError before anything is launched."""
    X, operator = _operator(X, operator, "whiten_l2_rows")
    n = X.shape[0]
    if n < 2:
        raise ValueError(f"whitening needs at least two rows, got {n}: one row has no covariance")
    if not bool(torch.isfinite(X).all()):
        raise ValueError("rows must be finite")
    dev = operator.device
    X = X.to(dev).float()
    mean, gram = operator.stats(X)
    W = whitening_matrix(gram.cpu().numpy(), n)
    return operator.apply(X, mean, torch.from_numpy(np.ascontiguousarray(W)).to(dev))


def label_centroids_rows(X, labels, k: int, *, operator=None):
    """The unit mean of the rows of every label c < k [REF diar_diag.py:379-382] -> (centres f32 [k, D], count int32 [k]) on the
    operator's device.  Labels outside [0, k) are skipped; an empty label gives a zero row."""
    X, operator = _operator(X, operator, "label_centroids_rows")
    if not 1 <= int(k) <= 1024:
        raise ValueError(f"k must be in [1, 1024], got {k}")
    dev = operator.device
    labels = torch.as_tensor(labels).to(dev)
    if labels.shape != (X.shape[0],):
        raise ValueError(f"labels {tuple(labels.shape)} do not match the {X.shape[0]} rows")
    return operator.centroids(X.to(dev).float(), labels, int(k))
