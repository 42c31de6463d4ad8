"""utils.select_output (AIQMCrelease3/utils/utils.py:1-6), and np64 of the drop-in layer."""
from typing import Any, Callable, Sequence

import numpy as np
import torch


def np64(t) -> np.ndarray:
    """A tensor, array or nested list as a float64 host array."""
    return np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=np.float64)


def select_output(f: Callable[..., Sequence[Any]], argnum: int) -> Callable[..., Any]:
    def f_selected(*args, **kwargs):
        return f(*args, **kwargs)[argnum]
    if hasattr(f, "_aiqmc_network"):
        f_selected._aiqmc_network = f._aiqmc_network
        f_selected._aiqmc_selected = argnum
    return f_selected
