"""Device route for k-means: scikit-learn's `k_means` labels for many recordings in one launch.

`sklearn.cluster.k_means(X, k, random_state=rs, n_init=R)` centres the rows, runs R restarts of greedy k-means++ seeding and Lloyd
iterations, and keeps the restart of lowest inertia.  Everything random in it is a fixed number of uniform draws per restart
(one for the first centre, t = 2 + floor(ln k) for each further one), so the host draws them in advance (`kmeans_draws`, which
leaves the `RandomState` where scikit-learn leaves it) and `ops.kmeans_grouped` (`sd_kmeans_grouped_f64`, include/sd_hip_kmeans.h)
does the rest in f64: one workgroup per (recording, restart), a second small launch for the selection.  The labels are
scikit-learn's, integer for integer and in its numbering, wherever the input has no near-tie.

What falls back to the host, and is named in `info["fallback"]`:
* a recording in which some iteration leaves a cluster without rows (flag EMPTY): scikit-learn relocates the farthest rows then,
  in an order that depends on `argpartition`; it is redone by `sklearn.cluster.k_means` with the generator in the state it had
  before that recording's draws;
* k > 32 or more than 32 columns.
A row with NaN or inf raises ValueError, as scikit-learn does.

The launch is injectable (`launch=`): a callable `launch(X, first_row, ks, first, u, n_init, max_iter, tol)` ->
`(labels, chosen, inertia, iters, flags)` as numpy arrays (labels int32 [rows], the others one entry per recording).  The CPU tests
run the drivers' packing, draws, fallback and unpacking through the numpy statement of the entry.  There is no implicit CPU route:
without a launch, host rows are uploaded through the `device_rows` guard, which raises where no GPU is visible.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .device_rows import DeviceRoute

EMPTY, NONFINITE, BAD_K, BAD_DRAW, BAD_PROMISE = 1, 2, 4, 8, 16
MAX_K, MAX_DIM, MAX_INIT = 32, 32, 16
U_CENTRES, U_TRIALS = MAX_K - 1, 5        # u is padded to [recordings, n_init, 31, 5]: 2 + floor(ln 32) = 5


class DeviceKMeans(DeviceRoute):
    route, takes = "k-means", "the rows"


def kmeans_draws(random_state: np.random.RandomState, n: int, k: int, n_init: int = 10):
    """The random numbers `sklearn.cluster.k_means(X [n rows], k, random_state=random_state, n_init=n_init)` would draw, in its order,
    leaving `random_state` as it would: per restart one `random_sample` (`RandomState.choice(n, p=1/n)`: the index is the position of
    the sample in the normalised cumulative sum of p, side "right") and k - 1 times `uniform(size=t)`, t = 2 + floor(ln k).
    -> (first int32 [n_init], u f64 [n_init, k - 1, t])."""
    t = 2 + int(math.log(k))
    weight = np.ones(n)
    cdf = (weight / weight.sum()).cumsum()
    cdf /= cdf[-1]
    # `uniform(size=t)` is 0 + 1 * `random_sample(t)`, and the generator hands out the same doubles however the calls are cut up
    draws = random_state.random_sample(n_init * (1 + (k - 1) * t)).reshape(n_init, 1 + (k - 1) * t)
    first = cdf.searchsorted(draws[:, 0], side="right").astype(np.int32)
    return first, np.ascontiguousarray(draws[:, 1:]).reshape(n_init, k - 1, t)


def device_launch(X, first_row, ks, first, u, n_init, max_iter, tol):
    """The product launch: `ops.kmeans_grouped` on the device of X and ONE synchronisation, the copy of its five results."""
    from . import ops
    dev = X.device
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)     # noqa: E731
    out = ops.kmeans_grouped(X, up(first_row, np.int32), up(ks, np.int32), up(first, np.int32), up(u, np.float64), n_init, max_iter, tol,
                             max_k=int(max(ks)), max_rows=int(np.diff(first_row).max()))
    n_rows, G = X.shape[0], len(ks)
    # one copy: the five results packed into one f64 vector on the device (int32 values are exact in f64)
    packed = torch.cat([o.double() for o in out]).cpu().numpy()
    labels, chosen, inertia, iters, flags = np.split(packed, np.cumsum([n_rows, G, G, G]))
    return labels.astype(np.int32), chosen.astype(np.int32), inertia, iters.astype(np.int32), flags.astype(np.int32)


def _host(X, k, rs, n_init, max_iter, tol):
    from sklearn.cluster import k_means
    _, labels, inertia, iters = k_means(np.asarray(X, np.float64), k, random_state=rs, n_init=n_init, max_iter=max_iter, tol=tol,
                                        return_n_iter=True)
    return labels, float(inertia), int(iters)


def k_means_groups(X, sizes, ks, random_states, *, n_init: int = 10, max_iter: int = 300, tol: float = 1e-4, return_info: bool = False,
                   launch=None):
    """`sklearn.cluster.k_means(X_g, ks[g], random_state=random_states[g], n_init=n_init, max_iter=max_iter, tol=tol)[1]` for every
    recording g, X_g the next sizes[g] rows of X, in one launch and one host synchronisation.  X: f64 [rows, dim] on the device, or
    numpy rows, which are uploaded (RuntimeError where no GPU is visible).  `ks`: one int or one per recording, 2 <= k < sizes[g];
    `random_states`: one `RandomState` (or seed) per recording, or a single one that the recordings draw from in turn; every
    generator is left where scikit-learn would leave it.  -> a list of numpy int32 label vectors, and with `return_info` an info
    dict: "chosen" (the restart kept), "inertia", "iterations" (one entry per recording) and "fallback" (the recordings the host
    redid).  ValueError for a row that holds NaN or inf, and for a k outside [2, sizes[g])."""
    sizes = [int(s) for s in sizes]
    G = len(sizes)
    ks = [int(ks)] * G if np.ndim(ks) == 0 else [int(k) for k in ks]
    if len(ks) != G:
        raise ValueError(f"ks has {len(ks)} entries for {G} recordings")
    if np.ndim(random_states) == 0 or isinstance(random_states, np.random.RandomState):
        shared = random_states if isinstance(random_states, np.random.RandomState) else np.random.RandomState(random_states)
        states = [shared] * G
    else:
        states = [rs if isinstance(rs, np.random.RandomState) else np.random.RandomState(rs) for rs in random_states]
        if len(states) != G:
            raise ValueError(f"random_states has {len(states)} entries for {G} recordings")
    if not 1 <= int(n_init) <= MAX_INIT:
        raise ValueError(f"n_init={n_init} must lie in [1, {MAX_INIT}]")
    if max_iter < 1 or not tol >= 0:
        raise ValueError(f"max_iter={max_iter} tol={tol}")
    n_rows, dim = int(X.shape[0]), int(X.shape[1])
    if sum(sizes) != n_rows:
        raise ValueError(f"sizes add up to {sum(sizes)}, X has {n_rows} rows")
    for g, (n, k) in enumerate(zip(sizes, ks)):
        if not 2 <= k < n:
            raise ValueError(f"recording {g}: k={k} must lie in [2, {n}), the number of its rows")
    first_row = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    host = [g for g in range(G) if ks[g] > MAX_K] if dim <= MAX_DIM else list(range(G))
    on_host = set(host)
    on_device = [g for g in range(G) if g not in on_host]

    # the draws, in recording order; the state before each recording's draws is kept for the fallback
    before, first, u = [None] * G, np.zeros((G, n_init), np.int32), np.zeros((G, n_init, U_CENTRES, U_TRIALS))
    host_out = {}
    for g in range(G):
        if g not in on_host:
            before[g] = states[g].get_state()           # a copy of its own
            f, uu = kmeans_draws(states[g], sizes[g], ks[g], n_init)
            first[g], u[g, :, :uu.shape[1], :uu.shape[2]] = f, uu
        else:
            rows = X[first_row[g]:first_row[g + 1]]
            host_out[g] = _host(rows.cpu().numpy() if isinstance(rows, torch.Tensor) else rows, ks[g], states[g], n_init, max_iter, tol)

    labels = [None] * G
    info = {"chosen": [-1] * G, "inertia": [0.0] * G, "iterations": [0] * G, "fallback": sorted(host)}
    if on_device:
        if launch is None:
            if not isinstance(X, torch.Tensor):
                DeviceKMeans.guard("cuda" if torch.cuda.is_available() else "cpu")
                X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)).to("cuda")
            DeviceKMeans.guard(X)
            launch = device_launch
        if len(on_device) < G:                              # the recordings of the launch, packed
            keep = np.concatenate([np.arange(first_row[g], first_row[g + 1]) for g in on_device])
            Xd = X[torch.from_numpy(keep).to(X.device)] if isinstance(X, torch.Tensor) else np.asarray(X)[keep]
        else:
            Xd = X
        fr = np.concatenate([[0], np.cumsum([sizes[g] for g in on_device])]).astype(np.int64)
        lab, chosen, inertia, iters, flags = launch(Xd, fr, np.array([ks[g] for g in on_device], np.int32), first[on_device], u[on_device],
                                                    int(n_init), int(max_iter), float(tol))
        bad = [g for i, g in enumerate(on_device) if flags[i] & NONFINITE]
        if bad:
            raise ValueError(f"Input X contains NaN or infinity (recording(s) {bad})")
        broken = [g for i, g in enumerate(on_device) if flags[i] & ~(EMPTY | NONFINITE)]
        if broken:
            raise RuntimeError(f"sd_kmeans_grouped_f64 refused recording(s) {broken}: flags {[int(flags[on_device.index(g)]) for g in broken]}")
        for i, g in enumerate(on_device):
            if flags[i] & EMPTY:
                states_after = states[g].get_state()
                rs = np.random.RandomState()
                rs.set_state(before[g])
                rows = Xd[fr[i]:fr[i + 1]]
                host_out[g] = _host(rows.cpu().numpy() if isinstance(rows, torch.Tensor) else rows, ks[g], rs, n_init, max_iter, tol)
                states[g].set_state(states_after)       # the draws of every recording were made in advance: the generator stays past them
                info["fallback"] = sorted(info["fallback"] + [g])
            else:
                labels[g] = lab[fr[i]:fr[i + 1]].astype(np.int32)
                info["chosen"][g], info["inertia"][g], info["iterations"][g] = int(chosen[i]), float(inertia[i]), int(iters[i])
    for g, (lab_g, inertia_g, iters_g) in host_out.items():
        labels[g] = np.asarray(lab_g, np.int32)
        info["inertia"][g], info["iterations"][g] = inertia_g, iters_g
    return (labels, info) if return_info else labels


def k_means_rows(X, k: int, random_state, *, n_init: int = 10, max_iter: int = 300, tol: float = 1e-4, return_info: bool = False, launch=None):
    """`sklearn.cluster.k_means(X, k, random_state=random_state, n_init=n_init, max_iter=max_iter, tol=tol)[1]` on the device:
    `k_means_groups` for one recording -> numpy int32 labels (and the info of that recording: "chosen", "inertia", "iterations",
    "fallback" as a bool)."""
    labels, info = k_means_groups(X, [X.shape[0]], [k], [random_state], n_init=n_init, max_iter=max_iter, tol=tol, return_info=True,
                                  launch=launch)
    one = {"chosen": info["chosen"][0], "inertia": info["inertia"][0], "iterations": info["iterations"][0], "fallback": bool(info["fallback"])}
    return (labels[0], one) if return_info else labels[0]
