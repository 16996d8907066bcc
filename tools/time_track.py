#!/usr/bin/env python3
"""Time K15 (ops.track_neurons) alone, and a torch baseline beside it:
python tools/time_track.py [repeats] [frames]

Cases: K = 100 neurons, T = 4000 frames (``frames``), sigma = 3: 512x512x1 with search (6, 6, 0) and 512x512x2 with search
(6, 6, 1).  The frames are noise plus a constant (what the frames hold does not change the work: every region is filtered in
full), the predictions random inside the volume.  HIP events around the whole call, the wrapper's three output allocations
included.  The torch baseline is the plainest formulation of the same result on the same device: gather the regions of
2 (search + r) + 1 voxels per axis from the zero-padded frames (advanced indexing, 250 frames at a time to bound the memory),
conv3d with the same taps, one axis after the other, argmax per window -- no weights, no refinement, no amplitude: it does
less.  Three warm-up calls, then the median and the minimum of ``repeats`` (default 20); nothing is asserted about time.

Bytes: every search must read its region -- the gathered bytes K T region 4 -- but neighbouring regions overlap and a frame is
at most X Y Z 4 bytes, so what must come from HBM is at most the frames themselves (each line once, if L2 and the Infinity
Cache held a frame while its K searches run).  Both are printed with the share of the 8 TB/s HBM peak they amount to at the
measured time.
"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402

PEAK = 8.0e12


def timed(fn, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def torch_baseline(frames, sz, predict, sigma, search, chunk=250):
    X, Y, Z = sz
    T, K = frames.shape[0], predict.shape[0]
    r = int(math.ceil(3 * sigma))
    dev = frames.device
    tap = torch.exp(-torch.arange(-r, r + 1, dtype=torch.float32, device=dev) ** 2 / sigma ** 2)
    h = [s + r for s in search]
    c = torch.round(predict).long()                                          # (K, 3)
    off = [torch.arange(-h[d], h[d] + 1, device=dev) for d in range(3)]
    # indices into the padded volume (pad h[d] per side): c + h + off - h ... = c + off + h
    ix = (c[:, 0, None] + off[0][None, :] + h[0])[:, :, None, None]
    iy = (c[:, 1, None] + off[1][None, :] + h[1])[:, None, :, None]
    iz = (c[:, 2, None] + off[2][None, :] + h[2])[:, None, None, :]

    def run():
        best = torch.empty((K, T), dtype=torch.int64, device=dev)
        for t0 in range(0, T, chunk):
            n = min(chunk, T - t0)
            V = torch.nn.functional.pad(frames[t0:t0 + n].view(n, X, Y, Z), (h[2], h[2], h[1], h[1], h[0], h[0]))
            R = V[:, ix, iy, iz].reshape(n * K, 1, *[2 * v + 1 for v in h])   # (n K, 1, wx, wy, wz)
            for d in range(3):
                shape = [1, 1, 1, 1, 1]
                shape[2 + d] = 2 * r + 1
                R = torch.nn.functional.conv3d(R, tap.view(shape))
            best[:, t0:t0 + n] = R.reshape(n, K, -1).argmax(2).t()
        return best
    return run


def case(sz, search, repeats, T, K=100, sigma=3.0):
    X, Y, Z = sz
    P = X * Y * Z
    torch.manual_seed(0)
    frames = (0.1 + 0.002 * torch.randn((T, P), device="cuda")).contiguous()
    predict = torch.rand((K, 3), dtype=torch.float64, device="cuda") * torch.tensor([X - 1.0, Y - 1.0, Z - 1.0], dtype=torch.float64,
                                                                                     device="cuda")
    r = int(math.ceil(3 * sigma))
    region = 1
    for d in range(3):
        region *= min(sz[d], 2 * (search[d] + 1 + r) + 1)
    pos, amp, peak = ops.track_neurons(frames, sz, predict, shape_std=sigma, search=search, threshold=-1e30)
    found = int(torch.isfinite(pos).all(1).sum())
    full = timed(lambda: ops.track_neurons(frames, sz, predict, shape_std=sigma, search=search, threshold=-1e30), repeats)
    gathered, once = 4.0 * K * T * region, 4.0 * T * P
    print(f"{X}x{Y}x{Z}, K = {K}, T = {T}, sigma = {sigma:g}, search {tuple(search)}: {found} of {K * T} searches returned a position; "
          f"region at most {region} voxels")
    print(f"  K15 whole call: median {full[0]:.3f} ms, min {full[1]:.3f} ms", flush=True)
    print(f"  gathered reads {gathered / 1e9:.2f} GB = {gathered / (full[0] * 1e-3) / PEAK:.3f} of 8 TB/s at the median; the frames once "
          f"{once / 1e9:.2f} GB = {once / (full[0] * 1e-3) / PEAK:.3f} of 8 TB/s", flush=True)
    base = timed(torch_baseline(frames, sz, predict, sigma, search), max(3, repeats // 4))
    print(f"  torch gather + conv3d x3 + argmax: median {base[0]:.3f} ms, min {base[1]:.3f} ms", flush=True)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    case([512, 512, 1], (6, 6, 0), repeats, T)
    case([512, 512, 2], (6, 6, 1), repeats, T)


if __name__ == "__main__":
    main()
