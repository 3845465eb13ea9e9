"""The integer tables the device ops return, as host arrays."""

from __future__ import annotations

import numpy as np


def host_table(x, cols: int, dtype=np.int64) -> np.ndarray:
    """``x`` (a tensor on any device or an array) as a host array of ``dtype`` and shape [n, cols]; ``cols=0``: [n]."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x, dtype=dtype)
    return x.reshape(-1, cols) if cols else x.reshape(-1)
