"""``Demix/Traces.py`` of the reference: ``cleanTraces``, and the step after it, ``deconvolveTraces`` (K21).  The reference's body is half-translated MATLAB and does not parse;
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


def deconvolveTraces(traces, fps=None, decay_time=None, g=None, penalty=None, baseline=None, noise=None, baseline_percentile=10.0):
    """When did each neuron fire: the AR(1), non-negative deconvolution of traces (K, T) (K21, ``ops.deconvolve_traces``;
    tests/deconv_restatement.py is the definition) -> ``(c, s, info)``: the denoised calcium traces, the spikes
    ``s_t = c_t - g c_{t-1} >= 0`` and a dict with ``g``, ``penalty``, ``baseline``, ``noise``, ``rss``, ``n_valid``, ``n_pools``
    and ``ok`` per trace.  Frames that are not finite -- what ``cleanTraces`` masks -- carry no weight; the trace decays through
    them.

    decay_time   the indicator's decay time in seconds: ``g = exp(-1 / (decay_time fps))``; needs ``fps`` and excludes ``g``
    g            the decay per frame in (0, 1); with neither, every trace's own ``ac(2) / ac(1)`` is taken
    penalty      the weight of sum(s); None: per trace the one at which the residual reaches the noise level
    baseline     None: the ``baseline_percentile``-th percentile of the valid frames, which sits below the true baseline by a
                 fraction of the noise (a jointly optimised baseline is not offered)
    noise        None: 1.4826 MAD / sqrt(2) of the differences of adjacent frames

    Each of ``g``, ``penalty``, ``baseline``, ``noise`` is None, a number or one value per trace (NaN: estimate that one).  A trace
    that cannot be treated has ``ok`` False and NaN rows.  A numpy array comes back as numpy arrays, a CUDA tensor as CUDA tensors;
    the input is not modified."""
    if decay_time is not None:
        if g is not None:
            raise ValueError("deconvolveTraces: give g or decay_time, not both")
        if fps is None:
            raise ValueError("deconvolveTraces: decay_time is in seconds and needs fps")
        if not (float(decay_time) > 0 and float(fps) > 0):
            raise ValueError(f"deconvolveTraces: decay_time={decay_time}, fps={fps}")
        g = float(np.exp(-1.0 / (float(decay_time) * float(fps))))
    kw = dict(g=g, penalty=penalty, baseline=baseline, noise=noise, baseline_percentile=baseline_percentile)
    if isinstance(traces, torch.Tensor):
        if not traces.is_cuda:
            raise ValueError("deconvolveTraces: a tensor must live on the GPU (numpy arrays are taken from the host)")
        t = traces if traces.dtype == torch.float32 and traces.stride(-1) == 1 else traces.float().contiguous()
        c, s, info = ops.deconvolve_traces(t, **kw)
        info.pop("workspace")
        return c, s, info
    t = torch.from_numpy(np.ascontiguousarray(traces, dtype=np.float32)).cuda()
    c, s, info = ops.deconvolve_traces(t, **kw)
    info.pop("workspace")
    return c.cpu().numpy(), s.cpu().numpy(), {k: v.cpu().numpy() for k, v in info.items()}
