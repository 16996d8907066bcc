#!/usr/bin/env python3
"""Time K17 (dnmf_warp_pullback, the trilinear registered movie) beside K7 (dnmf_image_iwarp) with HIP events:
python tools/time_registered.py [repeats] [--quick]

512x512x1 with 4000 frames and 512x512x2 with 1000, warps off the identity by several voxels (shifts, affine and quadratic
terms), rows of 1 and of 3 channels.  Prints per case the best time of each kernel and K17's share of its HBM floor: 8 bytes per
voxel, channel and frame (one read, one write) at the 8 TB/s roof.  ``--quick``: 64 frames (a rehearsal of the script, not a
measurement)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402

HBM_ROOF = 8.0e12   # bytes / s


def displaced_beta(T, sz, shift=4.0, seed=0):
    """Per frame: shifts of up to ``shift`` voxels, affine terms that move a corner by up to 4 voxels, quadratic ones by up to 1
    (z pinned at Z == 1, and kept within the slab at Z == 2)."""
    g = torch.Generator().manual_seed(seed)
    size = float(max(sz[0], sz[1]))
    beta = torch.cat((torch.zeros(1, 3), torch.eye(3), torch.zeros(6, 3)), 0)[:, :, None].repeat(1, 1, T)
    scale = torch.tensor([shift, 4 / size, 4 / size, 0, 1 / size ** 2, 1 / size ** 2, 0, 1 / size ** 2, 0, 0])
    beta[:, :2] += (2 * torch.rand(10, 2, T, generator=g) - 1) * scale[:, None, None]
    if sz[2] > 1:
        beta[0, 2] += 0.3 * (2 * torch.rand(T, generator=g) - 1)
    return beta.contiguous().cuda()


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


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    quick = "--quick" in sys.argv
    for sz, T in (([512, 512, 1], 4000), ([512, 512, 2], 1000)):
        if quick:
            T = 64
        P = sz[0] * sz[1] * sz[2]
        beta = displaced_beta(T, sz)
        times = torch.arange(T, dtype=torch.int32, device="cuda")
        for nchan in (1, 3):
            torch.manual_seed(0)
            frames = torch.rand(T, nchan * P, device="cuda")
            out = torch.empty_like(frames)
            bad = torch.zeros(1, dtype=torch.int64, device="cuda")
            fell = torch.zeros(1, dtype=torch.int64, device="cuda")
            t17 = best(lambda: ops.warp_pullback(frames, None, sz, beta, times, out=out, nchan=nchan, count=bad), repeats)
            t7 = best(lambda: ops.image_iwarp(frames, None, sz, beta, times, out=out, nchan=nchan, count=fell), repeats)
            floor_ms = 8.0 * P * nchan * T / HBM_ROOF * 1e3
            print(f"{sz[0]}x{sz[1]}x{sz[2]} x {T} frames, nchan {nchan}: K17 {t17:.3f} ms ({floor_ms / t17:.2f} of the HBM floor of "
                  f"{floor_ms:.3f} ms; points without a solution {int(bad) // (repeats + 1)}), K7 {t7:.3f} ms (exhaustive points "
                  f"{int(fell) // (repeats + 1)})", flush=True)
            del frames, out


if __name__ == "__main__":
    main()
