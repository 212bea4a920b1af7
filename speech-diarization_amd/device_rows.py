"""What the four product operators of the device routes share (`cluster_gpu.DeviceOperator`, `ahc_gpu.DeviceSums`,
`hdbscan_gpu.DeviceRows`, `diag_gpu.DeviceDiag`): the device, one `ops.Workspace` kept between calls, the refusal of anything that is
not on the GPU, and `normalise`.  The rows they hand to the kernels follow the contract `ops.rows4` states.  The injectable operator
protocols are documented in each route's module and do not derive from this class: the CPU tests implement them in numpy.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops


class DeviceRoute:
    route, takes = "", "its rows"        # the words of the refusal: "the device <route> route takes <takes> as a GPU tensor"

    def __init__(self, device):
        self.device = self.guard(device)
        self.ws = ops.Workspace(self.device)

    @classmethod
    def guard(cls, where) -> torch.device:
        """The GPU device of a tensor or of a device name; anything else (a host tensor, an array, "cpu") raises."""
        dev = where.device if isinstance(where, torch.Tensor) else where
        if not isinstance(dev, (torch.device, str, int)) or torch.device(dev).type != "cuda":
            raise RuntimeError(f"the device {cls.route} route takes {cls.takes} as a GPU tensor; there is no CPU fallback")
        return torch.device(dev)

    def normalise(self, X: torch.Tensor) -> torch.Tensor:
        """Unit rows, a zero row left zero (sklearn `normalize`), f32 [N, D padded to a multiple of 4 with zero columns]."""
        Xn = ops.l2norm_rows(X, sklearn_zero_guard=True)
        pad = -Xn.shape[1] % 4
        return torch.nn.functional.pad(Xn, (0, pad)) if pad else Xn


def operator_for(X, operator, cls):
    """`operator` when one was injected; otherwise the product operator `cls` on the device of X, which must be a GPU tensor."""
    return operator if operator is not None else cls(cls.guard(X))


def upload_rows(X, refusal: str, device="cuda") -> torch.Tensor:
    """Host rows (or a tensor) as f32 on `device`, for the callers that hold numpy rows and have no operator injected.  There is no CPU
    fallback: a `device` that is not a GPU (None: the caller has none to offer), or no visible GPU, raises RuntimeError(refusal)."""
    if device is None or torch.device(device).type != "cuda" or not torch.cuda.is_available():
        raise RuntimeError(refusal)
    X = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
    return X.to(device, dtype=torch.float32)
