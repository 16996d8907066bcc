"""Time K22 (``ops.high_pass_frames``, the whole call) with HIP events at 512 x 512 x 1 x 4000 and 512 x 512 x 2 x 1000
frames, gSig 3 and 7, against the 8 B per voxel and frame HBM floor (one read, one write), and beside it the same filter as
torch would run it: symmetric (period-2N reflected) padding by indexing + ``conv2d`` with the same taps.

    python tools/time_high_pass.py [--reps 5] [--hbm-tbs 8.0]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402


def time_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def reflect_index(n, h, dev):
    m = torch.remainder(torch.arange(-h, n + h, device=dev), 2 * n)
    return torch.where(m < n, m, 2 * n - 1 - m)


def torch_filter(frames, sz, taps, piece=250):
    """Symmetric padding by indexing + conv2d, slice by slice (Z as the batch of a channel-free conv), in pieces of frames."""
    X, Y, Z = sz
    n = taps.shape[0]
    h = n // 2
    ix, iy = reflect_index(X, h, frames.device), reflect_index(Y, h, frames.device)
    w = taps.view(1, 1, n, n)
    out = torch.empty_like(frames)
    for f0 in range(0, frames.shape[0], piece):
        v = frames[f0:f0 + piece].view(-1, X, Y, Z).permute(0, 3, 1, 2).reshape(-1, 1, X, Y)
        r = torch.nn.functional.conv2d(v[:, :, ix][:, :, :, iy], w)
        out[f0:f0 + piece] = r.view(-1, Z, X, Y).permute(0, 2, 3, 1).reshape(-1, X * Y * Z)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM bandwidth the floor is stated against, TB/s")
    args = ap.parse_args()
    for sz, T in (((512, 512, 1), 4000), ((512, 512, 2), 1000)):
        P = sz[0] * sz[1] * sz[2]
        frames = torch.rand((T, P), device="cuda")
        out = torch.empty_like(frames)
        for gsig in (3, 7):
            taps = torch.from_numpy(ops.high_pass_taps(gsig).astype(np.float32)).cuda()
            m = int(np.count_nonzero(ops.high_pass_taps(gsig)))
            k22 = time_ms(lambda: ops.high_pass_frames(frames, sz, gsig, out=out), args.reps)
            ref = torch_filter(frames[:8], sz, taps)
            diff = float((ops.high_pass_frames(frames[:8], sz, gsig) - ref).abs().max())
            tt = time_ms(lambda: torch_filter(frames, sz, taps), max(1, args.reps // 2))
            floor = 8.0 * P * T / (args.hbm_tbs * 1e12) * 1e3
            print(json.dumps({"sz": list(sz), "frames": T, "gSig": gsig, "taps": m, "k22_ms": round(k22, 3),
                              "hbm_floor_ms": round(floor, 3), "floor_share": round(floor / k22, 4),
                              "gflops": round(2.0 * m * P * T / (k22 * 1e-3) / 1e9, 1), "torch_pad_conv2d_ms": round(tt, 3),
                              "max_abs_diff_to_torch": diff}), flush=True)


if __name__ == "__main__":
    main()
