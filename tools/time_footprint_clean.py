#!/usr/bin/env python3
"""Time K27 (dnmf_clean_footprints) with HIP events around the whole ``ops.clean_footprints`` call, beside its numpy definition
(tests/footprint_clean_restatement.py) on one CPU core, and compare the two results for equality in the same run:
python tools/time_footprint_clean.py [repeats] [--quick]

K = 100 Gaussian footprints (sigma 3, values below 0.02 set to 0) at random centres in 512x512x1, and K = 200 in 512x512x2; every
footprint gets 12 speckles of 0.05 .. 0.3 within 12 voxels of its centre and one pinhole, as an exact spatial solve leaves them.
The call is timed at its defaults with the boxes already made (``component_boxes``, margin 1) -- it still checks them on the host
and copies them to the device.  A timed window is as many calls between two events as take about 50 ms (at most INNER); the best
of ``repeats`` windows is printed.  The definition is timed once; it median-filters whole (X, Y, Z) columns, which is
most of its time.  ``--quick``: K = 12, 64x64x1 (a rehearsal of the script, not a measurement)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dnmf_amd import ops  # noqa: E402
import footprint_clean_restatement as R  # noqa: E402

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
    """ms per call -> (best window, calls per window, windows).  One call warms up, one sizes the window to about 50 ms."""
    fn()
    t1 = window(fn, 1)
    inner = max(1, min(INNER, int(50.0 / max(t1, 1e-3))))
    return min([t1] + [window(fn, inner) for _ in range(repeats)]), inner, repeats


def make(K, sz, seed):
    rng = np.random.RandomState(seed)
    X, Y, Z = sz
    pos = np.stack([rng.uniform(16, X - 16, K), rng.uniform(16, Y - 16, K), np.full(K, 0.5 * (Z - 1))], 1)
    A = torch.zeros((X * Y * Z, K), dtype=torch.float32, device="cuda")
    gx, gy, gz = torch.meshgrid(torch.arange(X), torch.arange(Y), torch.arange(Z), indexing="ij")
    grid = torch.stack((gx, gy, gz), 3).reshape(-1, 3).float().cuda()
    for k in range(K):
        A[:, k] = torch.exp(-((grid - torch.tensor(pos[k], dtype=torch.float32, device="cuda")) ** 2).sum(1) / 9.0)
    A[A < 0.02] = 0
    A4 = A.view(X, Y, Z, K)
    for k in range(K):
        c = np.round(pos[k]).astype(int)
        for _ in range(12):
            d = rng.randint(-12, 13, 2)
            A4[c[0] + d[0], c[1] + d[1], rng.randint(Z), k] = float(rng.uniform(0.05, 0.3))
        A4[c[0], c[1], 0, k] = 0
    return A


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    quick = "--quick" in sys.argv
    torch.set_num_threads(1)
    for K, sz in ((100, (512, 512, 1)), (200, (512, 512, 2))):
        if quick:
            K, sz = 12, (64, 64, 1)
        A = make(K, sz, 0)
        boxes = ops.component_boxes(A, sz, floor=1e-3, margin=1).cpu()
        out = torch.empty_like(A)
        got, st = ops.clean_footprints(A, sz, boxes, out=out)
        t, inner, wins = best(lambda: ops.clean_footprints(A, sz, boxes, out=out), repeats)
        host = A.cpu().numpy()
        t0 = time.perf_counter()
        ref, rst = R.clean_footprints(host, sz, boxes.numpy())
        cpu = time.perf_counter() - t0
        same = np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)) and all(
            np.array_equal(st[n].cpu().numpy(), rst[n], equal_nan=True) for n in rst)
        nb = st["n_box"].double()
        print(f"K={K} {sz[0]}x{sz[1]}x{sz[2]}: boxes of {int(nb.min())} .. {int(nb.max())} voxels (mean {float(nb.mean()):.0f}), "
              f"{int(st['ok'].sum())} cleaned, kept {float(st['n_kept'].double().mean()):.0f} voxels a neuron of "
              f"{float((A > 0).sum(0).double().mean()):.0f}; clean_footprints {t:.3f} ms (best of {wins} windows of {inner} calls); "
              f"the numpy definition on one core {1e3 * cpu:.0f} ms; results equal: {same}")
        if quick:
            break


if __name__ == "__main__":
    main()
