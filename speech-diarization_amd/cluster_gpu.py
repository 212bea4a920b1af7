"""Device route for the two spectral steps: speaker count and spectral embedding without leaving the GPU.

`cluster.estimate_num_speakers` (dense f64 `eigvalsh` of the N x N Laplacian) and `cluster.spectral` (scikit-learn's
`SpectralClustering`) both need only a few extreme eigenpairs of

    S = D^-1/2 . max(K, 0) . D^-1/2

Here they come from a block Krylov iteration with Rayleigh-Ritz extraction whose only O(N^2) work is the product `S . V` for a
block V of 8 .. 32 vectors: `ops.affinity_apply` (`sd_affinity_apply_f32`, include/sd_hip_spectral.h), 8 to 16 passes over the f32
affinity exactly as `ops.cosine_affinity` left it on the device.  Opt-in: `diarize_audio(..., clustering="spectral_gpu")`;
`cluster.py` and the default `clustering="spectral"` are unchanged.

What runs where
* `S . V`, the row sums: HIP kernels, f32 (exact f32 products on the matrix cores, fixed summation order);
* the tall-skinny algebra, O(N b m): f64 `torch.matmul` on the operator's device (no `torch.linalg` call: no solver library needed);
* the m x m Rayleigh-Ritz `eigh` and the Gram factorisations of a new block: numpy f64 on the host (m <= block x steps);
* k-means over the N x k embedding: scikit-learn on the host, as in the host route; with `assign_labels="device"` the embedding
  stays on the device and `kmeans_gpu` labels it there (`sd_kmeans_grouped_f64`, include/sd_hip_kmeans.h).

The operator is injectable (`operator=`): an object with `n`, `device`, `degree(zero_diag)` and `apply(scale, V, zero_diag)` over
torch tensors.  `DeviceOperator` is the product one; the tests run the same solver on the CPU against a numpy operator.  There is no
implicit CPU route: without an operator a host tensor raises the product path's RuntimeError.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .device_rows import DeviceRoute

APPLY_BLOCKS = (8, 16, 24, 32)        # block widths sd_affinity_apply_f32 takes


class DeviceOperator(DeviceRoute):
    """max(K, 0) for an f32 affinity that lives on the GPU.  K is read in place on every pass and never copied, unless it is not
    symmetric: then 0.5 (K + K^T) is formed once, as the host functions do (`assume_symmetric=True` skips the check; the output
    of `ops.cosine_affinity` is exactly symmetric)."""

    route, takes = "spectral", "the affinity"

    def __init__(self, K: torch.Tensor, assume_symmetric: bool = False):
        super().__init__(self.guard(K))
        if K.dim() != 2 or K.shape[0] != K.shape[1]:
            raise ValueError(f"affinity must be square, got {tuple(K.shape)}")
        K = K if K.dtype == torch.float32 and (K.stride(1) == 1 or K.shape[0] <= 1) else K.float().contiguous()
        if not assume_symmetric and K.shape[0] > 1 and not torch.equal(K, K.T):
            K = 0.5 * (K + K.T)
        self.K = K
        self.n = K.shape[0]

    def degree(self, zero_diag: bool) -> torch.Tensor:
        return ops.affinity_degree(self.K, zero_diag)

    def apply(self, scale: torch.Tensor, V: torch.Tensor, zero_diag: bool) -> torch.Tensor:
        """V f32 [n, c], any c >= 1: padded with zero columns to the next block width the kernel takes, in pieces of at most 32."""
        out = []
        for c0 in range(0, V.shape[1], APPLY_BLOCKS[-1]):
            piece = V[:, c0:c0 + APPLY_BLOCKS[-1]]
            c = piece.shape[1]
            b = next(w for w in APPLY_BLOCKS if w >= c)
            if b != c:
                piece = torch.cat([piece, torch.zeros((self.n, b - c), dtype=piece.dtype, device=piece.device)], dim=1)
            out.append(ops.affinity_apply(self.K, scale, piece, zero_diag, ws=self.ws)[:, :c])
        return out[0] if len(out) == 1 else torch.cat(out, dim=1)


def _scale_of(deg: torch.Tensor) -> torch.Tensor:
    """1 / sqrt(deg), 1 for a row of degree 0 (scipy `csgraph_laplacian`: isolated nodes are divided by 1; the host
    `estimate_num_speakers` sets d[d <= 0] = 1)."""
    deg = deg.double()
    return torch.where(deg > 0, deg.clamp_min(1e-300).rsqrt(), torch.ones_like(deg))


def _orthonormalise(W: torch.Tensor, Q: torch.Tensor | None, ref: float, drop: float) -> torch.Tensor:
    """Columns of W (f64 [n, c]) made orthonormal to Q and to each other, through the eigen-decomposition of the Gram matrix (host,
    c x c) in two passes; directions whose norm after the first projection is below `drop` x `ref`, or that lose half of what is left
    in the second, are dropped (a converged basis leaves a rank-deficient block: a Cholesky factor would break down).  May return
    zero columns."""
    for p in range(2):
        if W.shape[1] == 0:
            return W
        if Q is not None and Q.shape[1]:
            W = W - Q @ (Q.T @ W)
        G = (W.T @ W).cpu().numpy()
        lam, Z = np.linalg.eigh(0.5 * (G + G.T))
        floor = (drop * ref) ** 2 if p == 0 else 0.25
        keep = lam > floor
        if not keep.any():
            return W[:, :0]
        T = torch.from_numpy(Z[:, keep] / np.sqrt(lam[keep])).to(W.device)
        W = W @ T
    return W


def top_eigenpairs(apply, n: int, nev: int, *, block: int = 24, tol: float = 1e-5, max_steps: int = 40, seed: int = 0,
                   device="cpu", drop: float = 1e-6):
    """The `nev` algebraically largest eigenpairs of a symmetric operator given as `apply(V) -> S V` (V f32 [n, c] on `device`;
    a torch tensor or a numpy array back): block Krylov with full re-orthogonalisation and Rayleigh-Ritz extraction.

    Every step applies the operator to the newest orthonormal block Q_j and stores S Q_j; T = Q^T S Q (m x m, symmetrised) is
    diagonalised on the host, and the residuals ||S u - theta u|| of the wanted Ritz pairs come from the stored blocks at no extra
    pass.  The iteration stops when the largest of them is <= `tol` (relative to max |theta|, at least 1), when the Krylov space
    is exhausted (no direction of the new block survives `_orthonormalise`: the Ritz pairs are then exact up to the operator's
    own rounding), or after `max_steps` passes.  The start block is drawn on the host from `numpy.random.default_rng(seed)`.

    -> (theta f64 [nev] descending (numpy), U f64 [n, nev] on `device` with orthonormal columns, info) with
    info = {"passes", "residual", "basis"}."""
    nev = min(int(nev), n)
    if nev <= 0 or n <= 0:
        return np.zeros(0), torch.zeros((n, 0), dtype=torch.float64, device=device), {"passes": 0, "residual": 0.0, "basis": 0}
    b = max(1, min(max(block, nev), n))
    rng = np.random.default_rng(seed)
    Qj = _orthonormalise(torch.from_numpy(rng.standard_normal((n, b))).to(device), None, np.sqrt(n), 1e-12)
    Q = Qj
    SQ = torch.zeros((n, 0), dtype=torch.float64, device=device)
    passes, resid = 0, float("inf")
    theta, Zw = np.zeros(0), None
    while True:
        W = torch.as_tensor(apply(Qj.float())).to(device=device, dtype=torch.float64)
        passes += 1
        SQ = torch.cat([SQ, W], dim=1)
        T = (Q.T @ SQ).cpu().numpy()
        lam, Z = np.linalg.eigh(0.5 * (T + T.T))
        order = np.argsort(lam)[::-1][:nev]
        theta, Zw = lam[order], torch.from_numpy(np.ascontiguousarray(Z[:, order])).to(device)
        have = len(order) == nev
        R = SQ @ Zw - (Q @ Zw) * torch.from_numpy(theta).to(device)
        resid = float(R.norm(dim=0).max()) / max(1.0, float(np.abs(lam).max()))
        if (have and resid <= tol) or passes >= max_steps or Q.shape[1] >= n:
            break
        Qj = _orthonormalise(W, Q, max(1.0, float(W.norm(dim=0).max())), drop)
        if Qj.shape[1] == 0:
            break
        Qj = Qj[:, :n - Q.shape[1]]
        Q = torch.cat([Q, Qj], dim=1)
    return theta, Q @ Zw, {"passes": passes, "residual": resid, "basis": int(Q.shape[1])}


def _operator(K, operator, assume_symmetric):
    return operator if operator is not None else DeviceOperator(K, assume_symmetric)


def _n_of(K, operator) -> int:
    if operator is not None:
        return int(operator.n)
    if K.dim() != 2 or K.shape[0] != K.shape[1]:
        raise ValueError(f"affinity must be square, got {tuple(K.shape)}")
    return int(K.shape[0])


def estimate_num_speakers(K, min_speakers: int, max_speakers: int, *, operator=None, assume_symmetric: bool = False,
                          block: int = 24, tol: float = 1e-5, max_steps: int = 40, seed: int = 0, return_info: bool = False):
    """`cluster.estimate_num_speakers` for an affinity on the GPU: the eigengap of I - D^-1/2 A D^-1/2, A = max(K, 0) with its
    diagonal, degrees including the diagonal, over the `hi + 1` smallest eigenvalues, clamped to [min, max]; the same early
    returns.  The `hi + 1` smallest Laplacian eigenvalues are 1 - the largest of S (`top_eigenpairs`)."""
    n = _n_of(K, operator)
    lo, hi = max(1, min_speakers), max(1, min(max_speakers, n))
    if hi <= lo:
        k = min(lo, hi) if n >= lo else max(1, n)
        return (k, {"passes": 0, "residual": 0.0, "basis": 0}) if return_info else k
    op = _operator(K, operator, assume_symmetric)
    scale = _scale_of(op.degree(False)).float()
    theta, _, info = top_eigenpairs(lambda V: op.apply(scale, V, False), n, hi + 1, block=block, tol=tol, max_steps=max_steps,
                                    seed=seed, device=op.device)
    ev = np.sort(1.0 - theta)[: hi + 1]
    gaps = np.diff(ev)
    k = int(np.argmax(gaps[lo - 1: hi]) + lo)
    info["eigenvalues"] = ev
    return (k, info) if return_info else k


def spectral_embedding(K, n_components: int, *, operator=None, assume_symmetric: bool = False, block: int = 24, tol: float = 1e-5,
                       max_steps: int = 40, seed: int = 0, on_device: bool = False):
    """The N x n_components rows scikit-learn's spectral clustering hands to k-means (see `spectral`) -> (numpy f64, info); with
    `on_device` the f64 tensor on the operator's device, not copied out."""
    op = _operator(K, operator, assume_symmetric)
    n = op.n
    deg = op.degree(True).double()
    scale = _scale_of(deg)
    _, U, info = top_eigenpairs(lambda V: op.apply(scale.float(), V, True), n, n_components, block=block, tol=tol,
                                max_steps=max_steps, seed=seed, device=op.device)
    emb = U * scale[:, None]                                     # x / dd, dd = sqrt(deg), 1 for isolated rows
    top = emb.abs().argmax(dim=0)
    sign = torch.sign(emb[top, torch.arange(emb.shape[1], device=emb.device)])
    emb = emb * torch.where(sign == 0, torch.ones_like(sign), sign)
    return (emb.contiguous() if on_device else emb.cpu().numpy()), info


def spectral(K, n_speakers: int, random_state: int = 0, *, operator=None, assume_symmetric: bool = False, block: int = 24,
             tol: float = 1e-5, max_steps: int = 40, seed: int = 0, return_info: bool = False, assign_labels: str = "sklearn",
             kmeans_launch=None):
    """`cluster.spectral` for an affinity on the GPU: what scikit-learn 1.7's
    `SpectralClustering(n_clusters, affinity="precomputed", assign_labels="kmeans", random_state=random_state).fit_predict(A)`
    computes for A = max(sym(K), 0), restated over the device operator.  The internals mirrored, in order:

    1. `sklearn.manifold._spectral_embedding(A, n_components=n_clusters, eigen_solver=None -> "arpack", drop_first=False)`:
       `scipy.sparse.csgraph.laplacian(A, normed=True, return_diag=True)` ignores the diagonal of A, takes the degrees without it and
       dd = sqrt(deg) with 1 for isolated rows; `_set_diag(laplacian, 1)` puts 1 on the whole diagonal: L = I - S;
    2. `eigsh(-L, k, sigma=1.0, which="LM")` and `diffusion_map.T[n_components::-1]`: the unit eigenvectors of the k smallest
       eigenvalues of L in ascending order = the k largest of S in descending order (here: `top_eigenpairs`);
    3. `embedding / dd`;
    4. `sklearn.utils.extmath._deterministic_vector_sign_flip`: each vector's largest-magnitude entry made positive;
    5. `sklearn.cluster.k_means(maps, n_clusters, random_state=rs, n_init=10)` on the host, where `rs` is the SAME
       `check_random_state(random_state)` instance `_init_arpack_v0` has already drawn N uniform numbers from for ARPACK's start
       vector: that draw is repeated here so that k-means sees the generator in the same state.

    `assign_labels="device"`: step 5 on the device.  The embedding is not copied out; after the N draws of `_init_arpack_v0` the
    random numbers of the k-means are drawn in advance (`kmeans_gpu.kmeans_draws`) and `kmeans_gpu.k_means_rows` returns
    scikit-learn's labels from one launch (`kmeans_launch`: its injectable `launch`, for the tests on the CPU).  The default
    "sklearn" is the host call above.  The labels of the two are equal, integer for integer, wherever the embedding has no near-tie
    (DESIGN.md section 23); `info["kmeans"]` says which restart was kept and whether the host had to redo it.  Measured at
    N = 7 609, k = 8 the whole call takes 14.8 ms with the device labels against 25.9 ms (profiles/kmeans_timing.json).  One
    recording runs on n_init workgroups only: at 50 000 rows of a 12-column embedding the device labels (134 ms) are no faster
    than scikit-learn on 16 host threads (95 to 157 ms); the gain is in the grouped launch over many recordings.

    Early returns as in `cluster.spectral`.  Labels agree with the host route whenever the eigenvectors are well separated from the
    rest of the spectrum (they differ from ARPACK's by ~1e-7, and k-means is a discontinuous function of its input)."""
    if assign_labels not in ("sklearn", "device"):
        raise ValueError(f"assign_labels={assign_labels!r}: 'sklearn' or 'device'")
    n = _n_of(K, operator)
    info = {"passes": 0, "residual": 0.0, "basis": 0}
    if n == 0:
        labels = np.zeros(0, dtype=int)
    elif n_speakers <= 1 or n <= n_speakers:
        labels = np.zeros(n, dtype=int) if n_speakers <= 1 else np.arange(n)
    else:
        emb, info = spectral_embedding(K, n_speakers, operator=operator, assume_symmetric=assume_symmetric, block=block, tol=tol,
                                       max_steps=max_steps, seed=seed, on_device=assign_labels == "device")
        rs = np.random.RandomState(random_state)
        rs.uniform(-1, 1, n)                                     # _init_arpack_v0
        if assign_labels == "device":
            from . import kmeans_gpu
            labels, info["kmeans"] = kmeans_gpu.k_means_rows(emb, n_speakers, rs, n_init=10, return_info=True, launch=kmeans_launch)
        else:
            from sklearn.cluster import k_means
            _, labels, _ = k_means(emb, n_speakers, random_state=rs, n_init=10)
    return (labels, info) if return_info else labels
