#!/usr/bin/env python3
"""Time K21 (the spike deconvolution, dnmf_deconvolve_traces) with HIP events around the whole call, beside two CPU baselines in the
same run:
python tools/time_deconvolve.py [repeats] [--quick]

K = 100 traces of T = 4000 frames and K = 200 of T = 16 000 (the second keeps its pool records in the workspace), simulated spikes
at density 0.1 through g = e^-0.3 on a baseline of 1 with white noise 0.1; two modes: g, penalty and baseline given (one solve), and
g given with the penalty searched (about forty solves inside the kernel).  Beside them, on one CPU core: for the given penalty
``sklearn.isotonic.isotonic_regression`` per trace under the mapping x_t = c_t g^-t -- a compiled baseline for the same projection,
on the first min(T, 1000) frames of every trace only and scaled to T, since g^-2t leaves float64 beyond that -- and, for both modes,
the float64 numpy restatement (tests/deconv_restatement.py), timed on the first NCPU traces and scaled to K.  Also prints the largest
difference between K21's c and the restatement's on those NCPU traces.  ``--quick``: K = 8, T = 1000 (a rehearsal of the script,
not a measurement)."""
import os
import sys
import time

import numpy as np
import torch
from sklearn.isotonic import isotonic_regression

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dnmf_amd import ops  # noqa: E402
import deconv_restatement as DR  # noqa: E402

NCPU = 4
G = float(np.exp(-0.3))
LAM = 0.5


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
    rng = np.random.RandomState(seed)
    s = (rng.rand(K, T) < 0.1).astype(np.float64)
    c = np.zeros((K, T))
    for t in range(T):
        c[:, t] = (G * c[:, t - 1] if t else 0.0) + s[:, t]
    return (1.0 + c + 0.1 * rng.randn(K, T)).astype(np.float32)


def isotonic_all(x, lam, b):
    n = min(x.shape[1], 1000)
    t = np.arange(n)
    gt, g2t = G ** t, G ** (2 * t)
    for row in x:
        a, _ = DR.terms(row[:n], G, lam, b)
        np.maximum(isotonic_regression(a / gt, sample_weight=g2t, increasing=True), 0.0) * gt
    return x.shape[1] / n


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 3
    quick = "--quick" in sys.argv
    for K, T in ((100, 4000), (200, 16000)):
        if quick:
            K, T = 8, 1000
        x = make(K, T)
        xd = torch.from_numpy(x).cuda()
        ws = ops.deconvolve_traces(xd, g=G, penalty=LAM, baseline=1.0)[2]["workspace"]
        for name, opt in (("penalty given", dict(g=G, penalty=LAM, baseline=1.0)), ("penalty searched", dict(g=G))):
            out = ops.deconvolve_traces(xd, workspace=ws, **opt)
            tk = best(lambda: ops.deconvolve_traces(xd, workspace=ws, **opt), repeats)
            t0 = time.perf_counter()
            ref = DR.deconvolve_traces(x[:NCPU], **opt)
            tc = (time.perf_counter() - t0) / NCPU * K * 1e3
            diff = np.abs(out[0][:NCPU].cpu().numpy().astype(np.float64) - ref[0]).max()
            line = f"K={K} T={T} {name}: K21 {tk:.3f} ms; numpy restatement {tc:.0f} ms ({NCPU} traces scaled to {K})"
            if "penalty" in opt:
                t0 = time.perf_counter()
                scale = isotonic_all(x, LAM, 1.0)
                line += f"; sklearn isotonic_regression, one core, {(time.perf_counter() - t0) * scale * 1e3:.0f} ms"
            else:
                lam = out[2]["penalty"].cpu().numpy()
                line += f"; penalties {lam.min():.3f} .. {lam.max():.3f}"
            print(line + f"; largest difference of c {diff:.2e}", flush=True)
        if quick:
            break


if __name__ == "__main__":
    main()
