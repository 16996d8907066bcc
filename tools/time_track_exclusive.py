#!/usr/bin/env python3
"""Time K15x (ops.track_neurons_exclusive), and K15 (ops.track_neurons) beside it in the same run:
python tools/time_track_exclusive.py [repeats] [frames]

Cases: K = 100 neurons, T = 4000 frames (``frames``), sigma = 3, search (6, 6, Z - 1), 512x512x1 and 512x512x2, one and two
rounds, the order 0..K-1 in every frame.  Twice: with the predictions spread over the volume (few regions hold a neighbour),
and packed into a 60 x 60 patch (about 2 sigma between neighbours: every region holds several).  The frames are noise plus a
constant and the threshold is -1e30, so every search returns a position and every neuron is placed (what the frames hold
does not change the work of a search).  HIP events around the whole ``ops`` call, the wrapper's permutation check and
output allocations included.  A timed window is as many calls between two events as take about 50 ms; the best of
``repeats`` (default 10) windows is printed; nothing is asserted about time.

K15x runs T workgroups whose K R searches are sequential, K15 runs K T independent ones.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def best(fn, repeats):
    """ms per call: the best window.  One call warms up, one sizes the window to about 50 ms."""
    fn()
    t1 = window(fn, 1)
    inner = max(1, min(50, int(50.0 / max(t1, 1e-3))))
    return min([t1] + [window(fn, inner) for _ in range(repeats)])


def case(sz, repeats, T, K=100, sigma=3.0):
    X, Y, Z = sz
    torch.manual_seed(0)
    frames = (0.1 + 0.002 * torch.randn((T, X * Y * Z), device="cuda")).contiguous()
    search = (6, 6, Z - 1)
    order = torch.arange(K, dtype=torch.int32, device="cuda")[:, None].repeat(1, T).contiguous()
    print(f"{X}x{Y}x{Z}, K = {K}, T = {T}, sigma = {sigma:g}, search {search}")
    for name, extent in (("spread", (X - 1.0, Y - 1.0)), ("packed", (60.0, 60.0))):
        predict = torch.rand((K, 3), dtype=torch.float64, device="cuda") * torch.tensor([extent[0], extent[1], Z - 1.0],
                                                                                         dtype=torch.float64, device="cuda")
        kw = dict(shape_std=sigma, search=search, threshold=-1e30)
        ms15 = best(lambda: ops.track_neurons(frames, sz, predict, **kw), repeats)
        print(f"  {name}: K15 {ms15:.3f} ms", flush=True)
        for rounds in (1, 2):
            nsub = ops.track_neurons_exclusive(frames, sz, predict, order, rounds=rounds, **kw)[3]
            ms = best(lambda: ops.track_neurons_exclusive(frames, sz, predict, order, rounds=rounds, **kw), repeats)
            print(f"  {name}: K15x {rounds} round(s) {ms:.3f} ms = {ms / ms15:.1f} x K15, {1e3 * ms / (K * rounds):.2f} us per search of a "
                  f"frame's sequence; neighbours in a region: mean {float(nsub.float().mean()):.1f}, most {int(nsub.max())}", flush=True)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    case([512, 512, 1], repeats, T)
    case([512, 512, 2], repeats, T)


if __name__ == "__main__":
    main()
