"""``Demix/Traces.py`` of the reference: ``cleanTraces``.  The reference's body is half-translated MATLAB and does not parse;
what it describes is defined in tests/traces_restatement.py and computed by K20 (``ops.clean_traces``) on the GPU.  Its
``histogram_match`` is not here: its body concatenates 1-D arrays along an axis they lack."""
from __future__ import annotations

import numpy as np
import torch

from .. import ops


def _none(v):
    """The reference writes ``[]`` for "none"."""
    if v is None or (isinstance(v, (list, tuple)) and len(v) == 0):
        return None
    return v


def cleanTraces(traces, fps, sigma_threshold=10, detrend_mode=2, interp_method=None, smooth_method=None, smooth_window=None):
    """Clean up neural traces (K, T): remove the acquisition outliers and the bleaching, then scale to [0.05, 0.95] (or, with
    ``detrend_mode=3``, to dF/F0 units) -> ``(traces, scales, offsets)`` as the reference's docstring says.

    sigma_threshold  a single frame whose change on both sides exceeds this many standard deviations above the mean is removed
                     (None, [] or 0: keep them)
    detrend_mode     0 leave the data as they are, 1 one bleach curve for all traces, 2 one per trace, 3 one per trace and the
                     division by F0 = max(median over the traces of their 5th percentile, 1)
    interp_method    None / [] or 'linear': fill the missing frames between two valid ones
    smooth_method    None / [], 'movmean' or 'movmedian' over ``smooth_window`` frames

    A numpy array comes back as float32 numpy arrays (scales, offsets float64), a CUDA tensor as CUDA tensors.  The input is
    not modified (the reference writes into its argument)."""
    kw = dict(sigma_threshold=_none(sigma_threshold), detrend_mode=detrend_mode, interp_method=_none(interp_method),
              smooth_method=_none(smooth_method), smooth_window=_none(smooth_window))
    if isinstance(traces, torch.Tensor):
        if not traces.is_cuda:
            raise ValueError("cleanTraces: a tensor must live on the GPU (numpy arrays are taken from the host)")
        t = traces if traces.dtype == torch.float32 and traces.stride(-1) == 1 else traces.float().contiguous()
        out, scales, offsets, _ = ops.clean_traces(t, fps, **kw)
        return out, scales, offsets
    t = torch.from_numpy(np.ascontiguousarray(traces, dtype=np.float32)).cuda()
    out, scales, offsets, _ = ops.clean_traces(t, fps, **kw)
    return out.cpu().numpy(), scales.cpu().numpy(), offsets.cpu().numpy()
