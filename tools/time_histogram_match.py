#!/usr/bin/env python3
"""Time K25 (histogram_match, dnmf_histogram_match) with HIP events around the whole ``ops.histogram_match`` call, beside a torch
composition of the same computation in the same run:
python tools/time_histogram_match.py [repeats] [--quick]

K = 100 rows of Ta = Tb = 4000 samples and K = 200 of Ta = Tb = 16 000, at nbins = 100 and 1024; traces with transients on a
baseline, 1 % of the samples NaN, the reference in other units.  The composition, all on the GPU in float64: ``torch.sort`` of both
sides (what is not finite as NaN, which sorts last), a gather of the two samples of every quantile at the same integer indices and
``torch.lerp``, ``torch.linalg.lstsq`` of qb on [qa, 1] per row, the affine map and the rounding to fp32 -- 'regular' only, no
distance; its first half (the quantiles of both sides) is also timed alone, since the batched ``lstsq`` dominates the whole.  A
timed window is as many calls between two events as take about 50 ms (at most INNER); the best of ``repeats`` windows is printed,
with the largest difference between the two results.  A function whose single call takes over 0.2 s is timed on two single
calls only.  ``--quick``: K = 8, T = 1000 (a rehearsal of the script, not a measurement)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dnmf_amd import ops  # noqa: E402

INNER = 500


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def best(fn, repeats):
    """ms per call -> (best window, calls per window, windows).  One call warms up, one sizes the window to about 50 ms (at most
    INNER calls); a function whose single call takes over 0.2 s is timed on that call and one more, not ``repeats`` times."""
    fn()
    t1 = window(fn, 1)
    inner = max(1, min(INNER, int(50.0 / max(t1, 1e-3))))
    windows = repeats if t1 < 200.0 else 1
    return min([t1] + [window(fn, inner) for _ in range(windows)]), inner, windows


def make(K, T, seed):
    rng = np.random.RandomState(seed)
    x = rng.gamma(2.0, 1.0, (K, T)) * rng.uniform(0.2, 5.0, (K, 1)) + rng.uniform(1.0, 8.0, (K, 1)) + 0.1 * rng.randn(K, T)
    x[rng.rand(K, T) < 0.01] = np.nan
    return torch.from_numpy(x.astype(np.float32)).cuda()


def sorted_quantiles(x, nbins):
    x = x.double()
    fin = torch.isfinite(x)
    xs = torch.sort(torch.where(fin, x, torch.full_like(x, float("nan"))), dim=1).values
    n = fin.sum(dim=1, keepdim=True)
    num = torch.arange(nbins, device=x.device, dtype=torch.int64)[None, :] * (n - 1)
    lo = num // (nbins - 1)
    frac = (num % (nbins - 1)).double() / float(nbins - 1)
    hi = torch.minimum(lo + 1, n - 1)
    return torch.lerp(xs.gather(1, lo), xs.gather(1, hi), frac)


def composition(a, b, nbins):
    qa, qb = sorted_quantiles(a, nbins), sorted_quantiles(b, nbins)
    beta = torch.linalg.lstsq(torch.stack([qa, torch.ones_like(qa)], dim=2), qb[:, :, None]).solution[:, :, 0]
    return (a.double() * beta[:, :1] + beta[:, 1:]).float(), beta


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    quick = "--quick" in sys.argv
    for K, T in ((100, 4000), (200, 16000)):
        if quick:
            K, T = 8, 1000
        a, b = make(K, T, 0), 3.0 * make(K, T, 1) + 2.0
        out = torch.empty_like(a)
        for nbins in (100, 1024):
            got = ops.histogram_match(a, b, nbins, out=out)
            want = composition(a, b, nbins)
            diff = float(((got[1] - want[1]).abs() / want[1].abs()).max())
            timed = [best(lambda: ops.histogram_match(a, b, nbins, out=out), repeats),
                     best(lambda: (sorted_quantiles(a, nbins), sorted_quantiles(b, nbins)), repeats),
                     best(lambda: composition(a, b, nbins), repeats)]
            how = ["%.3f ms (best of %d windows of %d calls)" % (t, w, n) for t, n, w in timed]
            print(f"K={K} Ta=Tb={T} nbins={nbins}: K25 {how[0]}; torch sort + gather + lerp of both sides {how[1]}; the same + "
                  f"lstsq + map {how[2]}; largest relative difference of beta {diff:.1e}", flush=True)
        if quick:
            break


if __name__ == "__main__":
    main()
