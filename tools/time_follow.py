#!/usr/bin/env python3
"""Time K15c (ops.follow_neurons), and K15 (ops.track_neurons) unchained beside it in the same run:
python tools/time_follow.py [repeats] [frames]

Cases: K = 100 neurons, T = 4000 frames (``frames``), sigma = 3, 512x512x1 and 512x512x2: the chain with search (3, 3, Z - 1)
from anchor 0 (one direction walks all T frames, the other one frame: the longest chain a call can have) and from the middle
frame (two chains of T / 2), and K15 with search (6, 6, Z - 1) around fixed predictions.  The frames are noise plus a
constant and the threshold is -1e30, so every search returns a position and no chain is lost (what the frames hold does not
change the work of a search: every region is filtered in full).  momentum = 0: on noise a chain with momentum runs off and is
lost, and the recurrence costs the same either way.  HIP events around the whole ``ops`` call, the wrapper's
output allocations included.  A timed window is as many calls between two events as take about 50 ms; the best of
``repeats`` (default 10) windows is printed; nothing is asserted about time.

The chain runs 2 K workgroups whose T steps are sequential, K15 runs K T independent ones: the per-step time printed for the
chain (time / the frames of its longest chain) is the latency of one search -- region read, three passes, pick, refinement -- not a
throughput.
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
    start = torch.rand((K, 3), dtype=torch.float64, device="cuda") * torch.tensor([X - 1.0, Y - 1.0, Z - 1.0], dtype=torch.float64,
                                                                                   device="cuda")
    narrow, wide = (3, 3, Z - 1), (6, 6, Z - 1)
    print(f"{X}x{Y}x{Z}, K = {K}, T = {T}, sigma = {sigma:g}")
    for anchor in (0, T // 2):
        kw = dict(shape_std=sigma, search=narrow, anchor=anchor, threshold=-1e30)
        out = ops.follow_neurons(frames, sz, start, **kw)
        found = int(torch.isfinite(out["positions"]).all(1).sum())
        lost = int((out["lost_at"] >= 0).sum())
        ms = best(lambda: ops.follow_neurons(frames, sz, start, **kw), repeats)
        steps = max(T - anchor, anchor + 1)
        print(f"  K15c search {narrow}, anchor {anchor}: {ms:.3f} ms = {1e3 * ms / steps:.2f} us per step of the longest chain; "
              f"{found} of {K * T} rows found, {lost} chains lost", flush=True)
    ms = best(lambda: ops.track_neurons(frames, sz, start, shape_std=sigma, search=wide, threshold=-1e30), repeats)
    print(f"  K15 unchained, search {wide}: {ms:.3f} ms", flush=True)
    ms = best(lambda: ops.track_neurons(frames, sz, start, shape_std=sigma, search=narrow, threshold=-1e30), repeats)
    print(f"  K15 unchained, search {narrow}: {ms:.3f} ms", flush=True)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    case([512, 512, 1], repeats, T)
    case([512, 512, 2], repeats, T)


if __name__ == "__main__":
    main()
