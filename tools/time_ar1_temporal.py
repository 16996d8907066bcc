#!/usr/bin/env python3
"""Time K32 (the AR(1)-constrained trace update, ops.ar1_temporal) with HIP events around whole calls, beside the exact solver K4h
(ops.hals_temporal) and K4h followed by K21 (ops.deconvolve_traces) on the same Gram data, in the same run:
python tools/time_ar1_temporal.py [repeats] [--quick]

K = 100 neurons, T = 4000 frames and K = 200, T = 1000: synthetic Gram data on a band pattern (every neuron overlaps up to four
others) with its neighbour table of 8 columns, AR(1) traces through g = e^-0.3 on the baseline 1, SWEEPS sweeps each from C = 1.
A whole call of ops.ar1_temporal is timed: the colouring on the host, the float64 copy of the state, one launch a colour and a
sweep, the rounding back to fp32.  The best of ``repeats`` calls after one that warms up.  ``--quick``: K = 16, T = 500 (a
rehearsal of the script, not a measurement)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dnmf_amd import ops  # noqa: E402

G = float(np.exp(-0.3))
SWEEPS = 5
LAM = 0.3


def best(fn, repeats):
    times = []
    for _ in range(repeats + 1):                    # the first call warms up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return min(times[1:])


def make(K, T, seed=0):
    """G (T, K, K), r (T, K) fp32 CUDA on a band of half-width 2, the table (K, 8) int32, the planted traces (K, T)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    Gm = torch.zeros((T, K, K), dtype=torch.float32, device="cuda")
    k = torch.arange(K, device="cuda")
    Gm[:, k, k] = 1.0 + torch.rand((T, K), generator=gen, device="cuda")
    for d in (1, 2):
        off = 0.2 * torch.rand((T, K - d), generator=gen, device="cuda")
        Gm[:, k[:-d], k[d:]] = off
        Gm[:, k[d:], k[:-d]] = off
    rng = np.random.RandomState(seed)
    s = (rng.rand(K, T) < 0.1).astype(np.float64)
    c = np.zeros((K, T))
    for t in range(T):
        c[:, t] = (G * c[:, t - 1] if t else 0.0) + s[:, t]
    truth = torch.from_numpy(1.0 + c).to("cuda", torch.float32)
    r = torch.einsum("tkl,lt->tk", Gm, truth) + 0.1 * torch.randn((T, K), generator=gen, device="cuda")
    nbr = torch.stack([k + d for d in (-2, -1, 0, 1, 2)], 1)
    nbr = torch.where((nbr >= 0) & (nbr < K), nbr, torch.full_like(nbr, -1))
    nbr = torch.cat([nbr, torch.full((K, 3), -1, device="cuda", dtype=nbr.dtype)], 1).sort(1, descending=True).values
    return Gm, r.contiguous(), nbr.to(torch.int32).contiguous(), truth


def median_corr(C, truth):
    C, truth = C.double().cpu().numpy(), truth.double().cpu().numpy()
    return float(np.median([np.corrcoef(C[k], truth[k])[0, 1] for k in range(len(C))]))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 3
    quick = "--quick" in sys.argv
    for K, T in ((100, 4000), (200, 1000)):
        if quick:
            K, T = 16, 500
        Gm, r, nbr, truth = make(K, T)
        C0 = torch.ones((K, T), dtype=torch.float32, device="cuda")

        def ar1():
            return ops.ar1_temporal(Gm, r, C0.clone(), G, LAM, 1.0, sweeps=SWEEPS, nbr=nbr)

        def hals():
            return ops.hals_temporal(Gm, r, C0.clone(), SWEEPS, nbr=nbr)      # K4h skips the -1 padding as K32 does

        def hals_deconv():
            return ops.deconvolve_traces(hals(), g=G, penalty=LAM, baseline=1.0)

        Ca, _, info = ar1()
        Ch = hals()
        cd, _, dinfo = hals_deconv()
        ta, th, td = best(ar1, repeats), best(hals, repeats), best(hals_deconv, repeats)
        print(f"K={K} T={T} {SWEEPS} sweeps: K32 ar1_temporal {ta:.3f} ms ({info['n_colours']} colours, {SWEEPS * info['n_colours']} launches); "
              f"K4h hals_temporal {th:.3f} ms; K4h + K21 deconvolve_traces {td:.3f} ms; median correlation with the planted traces: "
              f"ar1 {median_corr(Ca, truth):.4f}, hals {median_corr(Ch, truth):.4f}, hals + deconvolution {median_corr(1.0 + cd, truth):.4f}",
              flush=True)
        if quick:
            break


if __name__ == "__main__":
    main()
