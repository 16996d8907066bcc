#!/usr/bin/env python3
"""Time K10 (dnmf_nearest_points through ops.nearest_points, with values) alone: python tools/time_nearest.py [repeats] [--quick]

Cases: flows of 512x512x1 volumes from warp_gather, scaled by (n + 1) / 2 * sz as the reference's spatial_pushforward does
(256 frames, identity beta and displaced beta: a shift plus a mild quadratic warp), 256x256x20 (16 frames, displaced), and a
degenerate cloud (65536 points in a 256 x 256 square plus one point 10^6 away: every point in one cell, O(N) per query).  The
queries are the voxel lattice (one set for every frame).  Prints ms per frame, points per second, K7 (ops.image_iwarp) on the
same frames for scale, and the bytes the implementation moves (below) against 8 TB/s.  --quick: the displaced 512x512x1 case
only, one timed call (the counter passes of tools/pmc_kernel.sh).

Bytes per point of a frame with Q = N (fp32 points): bounding box, count and scatter each read the point (3 x 12), the
(cell, rank) pair is written and read (16), the cell counts are zeroed, incremented, scanned and read by the scatter
(4 x 4), the record is written and read at least once (2 x 16), the query read (24), the value gathered (4), the index and
the value written (8): 136 B.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402
from oracle import dnmf_oracle as O  # noqa: E402

PEAK = 8.0e12
BYTES_PER_POINT = 3 * 12 + 16 + 4 * 4 + 2 * 16 + 24 + 4 + 8


def lattice(sz):
    return torch.from_numpy(O.voxel_lattice(sz).reshape(-1, 3)).to("cuda", torch.float64)


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3)
    return best


def report(name, B, N, Q, t, t7=None):
    moved = BYTES_PER_POINT * float(N) * B
    k7 = f"; K7 {t7 * 1e3 / B:.4f} ms per frame ({t / t7:.1f}x K7's time)" if t7 else ""
    print(f"{name}: {t * 1e3 / B:.4f} ms per frame, {N * B / t / 1e9:.3f} G points/s; {BYTES_PER_POINT} B/point: "
          f"{moved / t / 1e9:.0f} GB/s = {moved / t / PEAK:.3f} of 8 TB/s{k7}", flush=True)


def warp_case(name, sz, T, displaced, repeats, with_k7=True):
    beta = O.identity_beta(T)
    if displaced:
        rng = np.random.RandomState(1)
        base = np.array([3.0, 2e-2, 2e-2, 2e-2, 2e-4, 2e-4, 2e-4, 2e-4, 2e-4, 2e-4])
        beta += (rng.randn(10, 3, T) * base[:, None, None] * 0.3).astype(np.float32)
        beta[0, 0] += 2.5
        if sz[2] == 1:
            beta[:, 2] = O.identity_beta(T)[:, 2]
    b = torch.from_numpy(beta).cuda()
    P = int(np.prod(sz))
    times = list(range(T))
    _, grid = ops.warp_gather(torch.zeros((*sz, 1), device="cuda"), b, times, want_A_t=False)
    szt = torch.tensor([float(s) for s in sz], device="cuda")
    pts = (((grid + 1) / 2) * szt[None, None, None, :, None]).permute(4, 0, 1, 2, 3).reshape(T, P, 3).contiguous()
    del grid
    vals = torch.rand(T, P, device="cuda")
    q = lattice(sz)
    idx = torch.empty((T, P), dtype=torch.int32, device="cuda")
    out = torch.empty((T, P), device="cuda")
    t = timed(lambda: ops.nearest_points(pts, q, values=vals, out_index=idx, out=out), repeats)
    t7 = None
    if with_k7:
        o7 = torch.empty((T, P), device="cuda")
        t7 = timed(lambda: ops.image_iwarp(vals, None, sz, b, times, out=o7), repeats)
        print(f"  values different from K7's: {int((o7 != out).sum())} of {T * P} (near-ties)")
    report(name, T, P, P, t, t7)


def degenerate_case(repeats):
    rng = torch.Generator(device="cuda").manual_seed(2)
    N = 65536
    pts = torch.rand(1, N, 3, device="cuda", generator=rng) * torch.tensor([256.0, 256.0, 0.0], device="cuda")
    pts[0, 17] = torch.tensor([1e6, -1e6, 0.0])
    q = (torch.rand(N, 3, device="cuda", generator=rng) * 256).double()
    q[:, 2] = 0
    vals = torch.rand(1, N, device="cuda")
    t = timed(lambda: ops.nearest_points(pts, q, values=vals), repeats)
    report("degenerate: 65536 points in one cell (one outlier)", 1, N, N, t)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    if "--quick" in sys.argv:
        warp_case("512x512x1, 256 frames, displaced", [512, 512, 1], 256, True, 1, with_k7=False)
        return
    warp_case("512x512x1, 256 frames, identity", [512, 512, 1], 256, False, repeats)
    warp_case("512x512x1, 256 frames, displaced", [512, 512, 1], 256, True, repeats)
    warp_case("256x256x20, 16 frames, displaced", [256, 256, 20], 16, True, repeats)
    degenerate_case(repeats)


if __name__ == "__main__":
    main()
