#!/usr/bin/env python3
"""Time K14 (ops.detect_neurons) alone, and a torch baseline beside it:
python tools/time_detect.py [repeats]

Cases: 512x512x1 with K = 100 and 512x512x2 with K = 200 planted Gaussians (sigma = 3, amplitudes 0.99^k, noise 0.002), asked
for as many.  HIP events around the whole call (two filter passes, the tile table, the one-workgroup pursuit; the wrapper's
output allocations included, the median not: the background is passed), and around a call with K = 1, which is the filter,
the table and one round of the pursuit.  The C entry enqueues its four launches in one call, so the filter and the pursuit
are not timed apart: the K = 1 call stands for the filter (it overstates it by one round), and the pursuit's time per neuron
is the difference of the two calls over K - 1 -- an approximation, named as one where it is printed.  The torch baseline is what the kernel
replaces at its simplest: conv3d with the same taps, one axis after the other, then K times argmax plus a masked fill of the
exclusion ball (no refinement, no subtraction -- it does less).  Three warm-up calls, then the median and the minimum of
``repeats`` (default 20); nothing is asserted about time.
"""
import ctypes
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import _lib, ops  # noqa: E402


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


def planted(sz, K, sigma, seed=0):
    rng = np.random.RandomState(seed)
    centres = []
    while len(centres) < K:
        c = np.array([rng.uniform(0, sz[0] - 1), rng.uniform(0, sz[1] - 1), rng.uniform(0, sz[2] - 1)])
        if all(np.hypot(*(c[:2] - o[:2])) >= 3.2 * sigma for o in centres):
            centres.append(c)
    g = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device="cuda") for n in sz], indexing="ij")
    V = torch.zeros(tuple(sz), device="cuda")
    for k, c in enumerate(centres):
        V += 0.99 ** k * torch.exp(-((g[0] - c[0]) ** 2 + (g[1] - c[1]) ** 2 + (g[2] - c[2]) ** 2) / sigma ** 2)
    torch.manual_seed(seed)
    return (V + 0.002 * torch.randn_like(V)).contiguous(), np.array(centres)


def torch_baseline(V, K, sigma, md):
    r = int(math.ceil(3 * sigma))
    tap = torch.exp(-torch.arange(-r, r + 1, dtype=torch.float32, device=V.device) ** 2 / sigma ** 2)
    g = torch.meshgrid(*[torch.arange(n, dtype=torch.float32, device=V.device) for n in V.shape], indexing="ij")

    def run():
        R = V[None, None]
        for d in range(3):
            shape = [1, 1, 1, 1, 1]
            shape[2 + d] = 2 * r + 1
            pad = [0, 0, 0]
            pad[d] = r
            R = torch.nn.functional.conv3d(R, tap.view(shape), padding=pad)
        R = R[0, 0].clone()
        out = torch.empty((K,), dtype=torch.int64, device=V.device)
        for k in range(K):
            i = torch.argmax(R)
            out[k] = i
            x, y, z = i // (V.shape[1] * V.shape[2]), (i // V.shape[2]) % V.shape[1], i % V.shape[2]
            R.masked_fill_((g[0] - x) ** 2 + (g[1] - y) ** 2 + (g[2] - z) ** 2 <= md * md, float("-inf"))
        return out
    return run


def case(sz, K, repeats, sigma=3.0):
    V, centres = planted(sz, K, sigma)
    pos, amp, count = ops.detect_neurons(V, sz, K, shape_std=sigma, background=0.0)
    pos = pos.cpu().numpy()
    d = np.linalg.norm(pos[None, :, :2] - centres[:, None, :2], axis=2)
    print(f"{sz[0]}x{sz[1]}x{sz[2]}, K = {K}, sigma = {sigma:g}: {int(count)} found, {int((np.nanmin(d, 1) <= 1.2).sum())} of {K} planted "
          f"centres have a pick within 1.2 voxels")
    need = _lib.load().dnmf_detect_neurons_workspace((ctypes.c_int * 3)(*sz), K, sigma)
    ws = torch.empty(((need + 3) // 4,), dtype=torch.float32, device="cuda")
    full = timed(lambda: ops.detect_neurons(V, sz, K, shape_std=sigma, background=0.0, workspace=ws), repeats)
    one = timed(lambda: ops.detect_neurons(V, sz, 1, shape_std=sigma, background=0.0, workspace=ws), repeats)
    base = timed(torch_baseline(V, K, sigma, 2 * sigma), max(3, repeats // 4))
    print(f"  K14 whole call: median {full[0]:.3f} ms, min {full[1]:.3f} ms", flush=True)
    print(f"  K14 filter + table + one pick (K = 1): median {one[0]:.3f} ms, min {one[1]:.3f} ms -> pursuit about "
          f"{(full[0] - one[0]) / (K - 1) * 1e3:.2f} us per neuron (difference of the two calls)", flush=True)
    print(f"  torch conv3d x3 + {K} x (argmax, masked_fill): median {base[0]:.3f} ms, min {base[1]:.3f} ms", flush=True)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    case([512, 512, 1], 100, repeats)
    case([512, 512, 2], 200, repeats)


if __name__ == "__main__":
    main()
