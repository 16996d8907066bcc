"""``Demix/Traces.py`` of the reference: ``cleanTraces``, and the step after it, ``deconvolveTraces`` (K21).  The reference's body is half-translated MATLAB and does not parse;
what it describes is defined in tests/traces_restatement.py and computed by K20 (``ops.clean_traces``) on the GPU.  Its
``histogram_match`` is K25 (``ops.histogram_match``): one line of its body is broken (it concatenates 1-D arrays along an axis
they lack where the design matrix was meant); what the rest states is defined in tests/histmatch_restatement.py."""
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


def detrend_df_f(traces, window, stride=None, percentile=8.0, mode='df', offset=0.0):
    """Traces (K, T) or (T,) read against their own running baseline (K31, ``ops.running_quantile`` and ``ops.baseline_apply`` on
    the traces as a movie of K voxels; tests/dff_restatement.py is the definition) -> ``(traces_out, baseline)``, both like
    ``traces``.  The baseline is, per trace, the ``percentile`` of every window of ``window`` frames, one every ``stride`` frames
    (None: a quarter of the window; 1: an exact running percentile filter), joined by straight lines between the window
    centres and flat outside them; ``mode``: ``'df'`` y - F0, ``'dff'`` (y - F0) / (F0 + offset), ``'dfsqrtf'``, ``'baseline'``.
    Frames that are not finite -- what ``cleanTraces`` masks -- are left out of their windows and stay NaN.  What CaImAn's
    ``detrend_df_f`` does to its traces, with three differences: linear instead of cubic interpolation between the knots, windows
    clamped at the two ends instead of padded, and an interpolated (``method='linear'``) percentile; the background ``b f`` is not
    added to the baseline.  A numpy array comes back as float32 numpy arrays, a CUDA tensor as CUDA tensors; the input is not
    modified."""
    if not 0.0 <= float(percentile) <= 100.0:
        raise ValueError(f"detrend_df_f: percentile must lie in [0, 100], got {percentile!r}")
    tensors = isinstance(traces, torch.Tensor)
    if tensors and not traces.is_cuda:
        raise ValueError("detrend_df_f: a tensor must live on the GPU (numpy arrays are taken from the host)")
    t = traces.float() if tensors else torch.from_numpy(np.ascontiguousarray(traces, dtype=np.float32)).cuda()
    single = t.dim() == 1
    if t.dim() not in (1, 2):
        raise ValueError(f"detrend_df_f: traces are (K, T) or (T,), got {tuple(t.shape)}")
    K, T = (1, t.shape[0]) if single else t.shape
    rows = torch.empty((T, K), dtype=torch.float32, device=t.device)          # (T, K): a movie of K voxels
    rows.copy_((t[None, :] if single else t).t())
    sz = (K, 1, 1)
    knots = ops.running_quantile(rows, sz, window, stride, float(percentile) / 100.0)
    out = ops.baseline_apply(rows, sz, knots["value"], knots["centres"], mode, offset).t().contiguous()
    base = ops.baseline_apply(rows, sz, knots["value"], knots["centres"], "baseline").t().contiguous()
    if single:
        out, base = out[0], base[0]
    return (out, base) if tensors else (out.cpu().numpy(), base.cpu().numpy())


def histogram_match(a, b, nbins, type):
    """The moving trace ``a`` rescaled so that its histogram resembles that of the reference trace ``b`` (K25,
    ``ops.histogram_match``; tests/histmatch_restatement.py is the definition) -> ``(atransform, distance)``.  The ``nbins``
    quantiles of both are taken at ``linspace(0, 1, nbins)`` over their finite samples, the quantiles of ``b`` are regressed on
    ``[quantiles of a, 1]`` -- ``type='regular'``: least squares; ``'non-negative'``: with both coefficients >= 0, as ``nnls``
    would -- and ``atransform = a beta0 + beta1``, NaN where ``a`` is not finite.  ``distance`` is the RMS mismatch of the matched
    quantiles (the reference declares a histogram distance and returns NaN).  The two traces need neither the same length nor
    the same missing frames.

    a 1-D and b 1-D: ``atransform`` like ``a`` and a scalar distance.  a (K, Ta) and b (K, Tb) or (Tb,), one reference for
    all: (K, Ta) and (K,).  A row without a finite sample on either side comes back NaN.  A numpy array comes back as numpy
    arrays (``atransform`` float32, ``distance`` float64), a CUDA tensor as CUDA tensors; the input is not modified."""
    if type not in ("regular", "non-negative"):
        raise ValueError(f"histogram_match: type={type!r}: 'regular' or 'non-negative'")
    tensors = isinstance(a, torch.Tensor)
    if tensors and not a.is_cuda:
        raise ValueError("histogram_match: a tensor must live on the GPU (numpy arrays are taken from the host)")

    def rows(x):
        if isinstance(x, torch.Tensor):
            x = x.to("cuda")
            return x if x.dtype == torch.float32 and x.stride(-1) == 1 else x.float().contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    ta, tb = rows(a), rows(b)
    single = ta.dim() == 1
    if single and tb.dim() != 1:
        raise ValueError(f"histogram_match: a is one trace, b must be one too, got {tuple(tb.shape)}")
    out, _, distance, _ = ops.histogram_match(ta[None, :] if single else ta, tb, nbins, nonneg=type == "non-negative")
    if single:
        out, distance = out[0], distance[0]
    if tensors:
        return out, distance
    return out.cpu().numpy(), (float(distance) if single else distance.cpu().numpy())
