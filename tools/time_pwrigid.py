#!/usr/bin/env python3
"""Time K9 (dnmf_apply_pwrigid, the piecewise-rigid corrected movie) alone: python tools/time_pwrigid.py [repeats]

Cases: 512x512x1 and 512x512x2 at 1000 frames, 256x256x20 at 200 frames, with the patch geometry of bench.py's
position_initialiser extra (strides 3 size / 16, overlaps size / 16 in x and y; one window over z) and shifts of up to
+-4 voxels.  Prints ms per 1000 frames, the HBM bandwidth of the design floor and of the traffic the three steps move, and
the fraction of 8 TB/s.  Floors (bytes per voxel and frame): 16 for a prefilter pass plus an evaluation pass (read the frame,
write the coefficients, read them back, write the output); this build moves 8 more per filtered axis beyond the first
(24 for Z == 1, 32 for Z > 1).
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402

PEAK = 8.0e12


def run(size, Z, T, repeats):
    sz = [size, size, Z]
    P = size * size * Z
    gen = torch.Generator(device="cuda").manual_seed(7)
    frames = torch.rand(T, P, device="cuda", generator=gen)
    stride, overlap = (3 * size) // 16, size // 16
    st, ov = (stride, stride, 1), (overlap, overlap, Z - 1)
    dims, _ = ops.patch_grid(sz, st, ov)
    NP = int(dims.prod())
    shifts = ((torch.rand(T, NP, 3, device="cuda", generator=gen) - 0.5) * 8.0 * 10).round() / 10
    shifts[..., 2] *= 0.1 if Z > 1 else 0.0
    shifts = shifts.contiguous()
    out = torch.empty_like(frames)
    tsum = torch.zeros(P, device="cuda")
    tcount = torch.zeros(P, dtype=torch.int32, device="cuda")
    ops.apply_pwrigid(frames, shifts, sz, st, ov, 0.5, out=out, tsum=tsum, tcount=tcount)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.apply_pwrigid(frames, shifts, sz, st, ov, 0.5, out=out, tsum=tsum, tcount=tcount)
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e-3)
    vox = float(P) * T
    moved = 32.0 if Z > 1 else 24.0      # x pass, y pass, (z pass), evaluation: 8 B each
    floor_bw = 16.0 * vox / best
    print(f"{size}x{size}x{Z}, {T} frames, {NP} patches: {best * 1e3 * 1000.0 / T:.2f} ms per 1000 frames; "
          f"16 B/voxel floor: {floor_bw / 1e9:.0f} GB/s = {floor_bw / PEAK:.3f} of 8 TB/s; "
          f"moved ({moved:.0f} B/voxel): {moved * vox / best / 1e9:.0f} GB/s = {moved * vox / best / PEAK:.3f}", flush=True)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    run(512, 1, 1000, repeats)
    run(512, 2, 1000, repeats)
    run(256, 20, 200, repeats)


if __name__ == "__main__":
    main()
