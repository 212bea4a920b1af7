"""Shared by tests/test_hdbscan_grouped_rules.py (CPU) and tests/test_gpu_hdbscan_grouped.py: the numpy statement of the two grouped
entries of include/sd_hip_hdbscan.h (`sd_hdb_core_grouped_f32`, `sd_hdb_outgoing_grouped_f32`) from `hdbscan_ref.gram_f32`, a numpy
operator with the group mask for `hdbscan_gpu.hdbscan_rows_groups`, the two workspace formulas, and the recordings both files cluster."""
import numpy as np
import torch

import hdbscan_ref as H
from ahc_grouped_ref import band, group_of, promise_broken  # noqa: F401  (the band, `group` and its promises are the grouped AHC entry's)

TILE = 128
CHUNK = 8


def core_workspace_bytes(n, k, max_group):
    """ceil((2 W + 1) / 8) slots of k scores per padded row."""
    T, W = band(n, max_group)
    return -(-(2 * W + 1) // CHUNK) * TILE * T * k * 4


def outgoing_workspace_bytes(n, max_group):
    """(2 W + 2) slots of 128 T padded rows, a weight and an index each."""
    T, W = band(n, max_group)
    return (2 * W + 2) * TILE * T * 8


def _runs(group):
    group = np.asarray(group)
    edges = np.flatnonzero(np.concatenate(([True], group[1:] != group[:-1], [True])))
    return zip(edges[:-1], edges[1:])


def core_grouped_from_gram(G, k, group):
    """`hdbscan_ref.core_from_gram` on the block of every group alone; -inf for a row with fewer than k others in its group."""
    core = np.full(len(group), -np.inf, G.dtype)
    for a, b in _runs(group):
        if b - a > k:
            core[a:b] = H.core_from_gram(G[a:b, a:b], k)
    return core


def outgoing_grouped_from_gram(G, core, comp, group):
    """`hdbscan_ref.outgoing_from_gram` on the block of every group alone, nn shifted to an index into all rows (-1 stays -1)."""
    n = len(group)
    nn, best = np.full(n, -1, np.int32), np.full(n, -np.inf, G.dtype)
    core, comp = np.asarray(core), np.asarray(comp)
    for a, b in _runs(group):
        g_nn, g_best = H.outgoing_from_gram(G[a:b, a:b], core[a:b], comp[a:b])
        nn[a:b] = np.where(g_nn >= 0, g_nn + a, -1)
        best[a:b] = g_best
    return nn, best


class NumpyGroupedRows(H.NumpyRows):
    """`hdbscan_gpu.DeviceRows`' interface over CPU torch tensors, the grouped passes included; `passes` counts every kind of pass.
    The Gram of all rows is formed once; a recording's block of it is NOT promised to be the bits of the Gram of the recording alone
    (BLAS blocks differently), so `alone(a, b)` hands out an operator for rows a .. b that reads the same block: both runs of a
    comparison then see the same scores, which is the property the kernels are specified to have."""

    def core_grouped(self, rows, k, group, max_group):
        self.passes += 1
        g = group.numpy()
        core = core_grouped_from_gram(self._G(rows), k, g).astype(np.float32)
        return torch.from_numpy(core), torch.tensor([int(promise_broken(g, max_group))], dtype=torch.int32)

    def outgoing_grouped(self, rows, core, comp, group, max_group):
        self.passes += 1
        g = group.numpy()
        nn, best = outgoing_grouped_from_gram(self._G(rows), core.numpy(), comp.numpy(), g)
        return torch.from_numpy(nn), torch.from_numpy(best.astype(np.float32)), torch.tensor([int(promise_broken(g, max_group))], dtype=torch.int32)

    def alone(self, all_rows, a, b):
        return _BlockRows(self._G(all_rows)[a:b, a:b])


class _BlockRows(H.NumpyRows):
    def __init__(self, G):
        super().__init__()
        self._block = G

    def _G(self, rows):
        assert rows.shape[0] == self._block.shape[0]
        return self._block


# ------------------------------------------------------------------ the recordings of the driver tests

def identical_rows(m, d=192):
    """m copies of one unit row: every weight ties with every other."""
    v = np.zeros((1, d), np.float32)
    v[0, :3] = (0.6, 0.8, 0.0)
    return np.repeat(v, m, axis=0)


def driver_recordings():
    """[(name, unit rows f32 [m, 192])]: planted recordings (the recorded tie input `hdbscan_ref.TIED_INPUT` among them) mixed with
    sizes 0, 1, 2, 3 and 129 and a recording of identical rows.  No boundary but the first lies on a tile edge."""
    shape, seed = H.TIED_INPUT
    tied = H.planted(shape[0], shape[1], shape[2], seed, shape[3])
    p300, p700 = H.planted(300, 4, 0.6, 0, 0), H.planted(700, 3, 0.5, 1, 0)
    small = H.planted(129, 3, 0.5, 5, 4)
    return [("planted300", p300), ("two", small[:2].copy()), ("empty", small[:0].copy()), ("tied1000", tied), ("one", small[7:8].copy()),
            ("three", small[10:13].copy()), ("identical40", identical_rows(40)), ("planted129", small), ("planted700", p700)]
