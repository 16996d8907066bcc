#!/usr/bin/env python3
"""Time K29 (dnmf_colour_normal_eqs, dnmf_colour_solve) and the whole ``MultiChannelDNMF.update_colours`` with HIP events, beside
torch's einsum in the same run:
python tools/time_colours.py [repeats] [--quick]

The config-5 shard -- 512x512x1, 3 channels, K = 200, 1000 frames -- and K = 100 with 4000 frames.  ``colour_normal_eqs`` is timed
on the G and r the model's Gram kernel makes, beside ``torch.einsum('tkl,kt,lt->kl', G, C, C)`` in fp32 (no float64, no fixed order);
``colour_solve`` with 10 sweeps on its result; ``update_colours(dry_run=True)`` as a whole, Gram passes of the three channels
included.  A timed window is as many calls between two events as take about 50 ms (at most INNER); the best of ``repeats`` windows
is printed.  ``--quick``: 64x64, K = 12, 50 frames (a rehearsal of the script, not a measurement)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dnmf_amd import ops  # noqa: E402
from dnmf_amd.Demix.dNMF import MultiChannelDNMF, ResidentLoader  # noqa: E402

INNER = 500
NC = 3


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def best(fn, repeats):
    """ms per call -> (best window, calls per window, windows).  One call warms up, one sizes the window to about 50 ms."""
    fn()
    t1 = window(fn, 1)
    inner = max(1, min(INNER, int(50.0 / max(t1, 1e-3))))
    return min([t1] + [window(fn, inner) for _ in range(repeats)]), inner, repeats


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    quick = "--quick" in sys.argv
    for K, T, size in ((200, 1000, 512), (100, 4000, 512)):
        if quick:
            K, T, size = 12, 50, 64
        sz = [size, size, 1]
        P = size * size
        rng = np.random.RandomState(0)
        pos = torch.from_numpy(rng.rand(K, 3) * np.array([size, size, 0.0])).float()
        colours = torch.from_numpy(0.3 + 0.7 * rng.rand(NC, K)).float()
        dn = MultiChannelDNMF(torch.tensor(sz), K, T, torch.ones(NC, K), positions=pos)
        dn.verbose = False
        dn.C = torch.from_numpy(0.2 + rng.rand(K, T)).float().cuda()
        A = dn.fp.A.reshape(P, K)
        frames = torch.empty((T, NC * P), dtype=torch.float32, device="cuda")
        for c in range(NC):
            torch.matmul(dn.C.t(), (A * colours[c].cuda()).t(), out=frames[:, c * P:(c + 1) * P])
        frames += 0.05 * torch.rand_like(frames)
        loader = ResidentLoader(frames, sz, 50)
        order = torch.arange(T, dtype=torch.int32, device="cuda")
        G, rs = None, []
        for c in range(NC):
            Gc, rc = dn._gram_rhs_one(dn.fp, frames[:, c * P:(c + 1) * P], order)
            G = Gc if G is None else G
            rs.append(rc)
        r = torch.stack(rs)
        del Gc, rs
        M, b, state = ops.colour_normal_eqs(G, r, dn.C)
        Me = torch.einsum('tkl,kt,lt->kl', G, dn.C, dn.C)
        dev = float((Me.double() - M).abs().max() / M.abs().max())
        out = (M, b)
        start = dn.colours.contiguous()
        sol = ops.colour_solve(M, b, start, sweeps=10)
        timed = [best(lambda: ops.colour_normal_eqs(G, r, dn.C, state=state, out=out), repeats),
                 best(lambda: torch.einsum('tkl,kt,lt->kl', G, dn.C, dn.C), repeats),
                 best(lambda: ops.colour_solve(M, b, start, sweeps=10), repeats)]
        del G, r
        timed.append(best(lambda: dn.update_colours(loader, sweeps=10, dry_run=True), repeats))
        res = dn.update_colours(loader, sweeps=10, dry_run=True)
        err = float((res["colours"].cpu() - colours / colours.max(0).values).abs().max())
        how = ["%.3f ms (best of %d windows of %d calls)" % (t, w, n) for t, n, w in timed]
        print(f"K={K} T={T} {size}x{size}x1, {NC} channels: colour_normal_eqs {how[0]}; torch.einsum('tkl,kt,lt->kl') in fp32 {how[1]} "
              f"(largest difference from M {dev:.1e} of its maximum); colour_solve, 10 sweeps {how[2]} (kkt {float(sol['kkt'].max()):.2e}); "
              f"update_colours {how[3]}; largest colour error after it {err:.3f}", flush=True)
        del dn, frames, loader
        torch.cuda.empty_cache()
        if quick:
            break


if __name__ == "__main__":
    main()
