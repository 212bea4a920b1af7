"""Shared by tests/test_ahc_grouped_rules.py (CPU) and tests/test_gpu_ahc_grouped.py: the numpy statement of the grouped nearest entry
(`sd_ahc_nearest_grouped_f32`, include/sd_hip_ahc.h), a numpy operator with the group mask for `ahc_gpu.ahc_cosine_groups`, the
workspace formula, and the recordings both files cluster."""
import numpy as np
import torch

import ahc_ref as A

TILE = 128


def band(n, max_group):
    """(T, W) of the header: the tiles of n rows, and how many tiles right of the diagonal a group of max_group rows reaches."""
    T = -(-n // TILE)
    return T, min(T - 1, -(-(max_group - 1) // TILE))


def workspace_bytes(n, max_group):
    """(2 W + 2) slots of 128 T padded rows, a score and an index each."""
    T, W = band(n, max_group)
    return (2 * W + 2) * TILE * T * 8


def group_of(sizes):
    return np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)


def promise_broken(group, max_group):
    """What `bad` reports: `group` decreases somewhere, or a group has more than max_group rows."""
    group = np.asarray(group)
    return bool((np.diff(group) < 0).any() or (len(group) > max_group and (group[:-max_group] == group[max_group:]).any()))


def nearest_grouped_f32(sums, inv_count, group):
    """`ahc_ref.nearest_f32` on the rows of every group alone, nn shifted to an index into all rows (-1 stays -1)."""
    group = np.asarray(group)
    n = len(group)
    nn, best = np.full(n, -1, np.int32), np.full(n, -np.inf, np.float32)
    edges = np.flatnonzero(np.concatenate(([True], group[1:] != group[:-1], [True])))
    for a, b in zip(edges[:-1], edges[1:]):
        g_nn, g_best = A.nearest_f32(sums[a:b], inv_count[a:b])
        nn[a:b] = np.where(g_nn >= 0, g_nn + a, -1)
        best[a:b] = g_best
    return nn, best


class NumpyGroupedSums(A.NumpySums):
    """`ahc_gpu.DeviceSums`' interface over CPU torch tensors, the grouped nearest included.  `passes` counts both kinds of pass."""

    def nearest_grouped(self, sums, inv_count, group, max_group):
        self.passes += 1
        g = group.numpy()
        nn, best = nearest_grouped_f32(sums.numpy(), inv_count.numpy(), g)
        return torch.from_numpy(nn), torch.from_numpy(best), torch.tensor([int(promise_broken(g, max_group))], dtype=torch.int32)


# ------------------------------------------------------------------ the recordings of the driver tests

TWO_ROWS = np.array([[1.0, 0.0, 0.0], [0.6, 0.8, 0.0]], np.float32)          # cosine 0.6: of tests/test_gpu_ahc.py's tiny inputs
DRIVER_FAMILIES = (400, 700, 1000)
DRIVER_THRESHOLDS = sorted({thr for rows, thr in A.DRIVER_PAIRS if rows in DRIVER_FAMILIES}, reverse=True)       # 0.3, 0.1, 0.0


def driver_recordings(thr):
    """[(family or None, rows f32 [m, 192])] clustered together at `thr`: every family of DRIVER_FAMILIES that `ahc_ref.DRIVER_PAIRS`
    holds at this threshold (400 at 0.3; 400, 700 at 0.1; all three at 0.0), and between them a 2-row recording (zero padded to the
    families' width), an empty one and a 1-row one."""
    fam = [(f, A.family_rows(f)[0]) for f in DRIVER_FAMILIES if (f, thr) in A.DRIVER_PAIRS]
    two = np.zeros((2, fam[0][1].shape[1]), np.float32)
    two[:, :3] = TWO_ROWS
    return fam[:1] + [(None, two)] + fam[1:2] + [(None, two[:0]), (None, fam[0][1][5:6].copy())] + fam[2:]
