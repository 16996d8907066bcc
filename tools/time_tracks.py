#!/usr/bin/env python3
"""Time K11 / K12 / K13 (ops.fit_quadratic_warp, ops.invert_quadratic_warp, ops.roi_signals) alone:
python tools/time_tracks.py [repeats]

Cases: K = 100 neurons, T = 4000 frames of 512x512x1 (the bench's volume), and K = 200, T = 1000 with rows of 3 channels of
512x512 (the multi-channel layout: K13 reads the first channel of every row, ld = 3 P).  The tracks come from K12 on a
near-identity beta, so K11 fits what K12 made.  The frames hold random values (K13's time does not depend on them).  Prints
ms per call and microseconds per frame; nothing is asserted about time.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402


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


def case(name, sz, K, T, nchan, repeats):
    rng = np.random.RandomState(0)
    P = int(np.prod(sz))
    amp = np.array([2.0, 1e-2, 1e-2, 1e-2, 1e-5, 1e-5, 1e-5, 1e-5, 1e-5, 1e-5])
    beta = np.concatenate((np.zeros((1, 3)), np.eye(3), np.zeros((6, 3))))[:, :, None] + rng.randn(10, 3, T) * amp[:, None, None]
    if sz[2] == 1:
        beta[:, 2] = [[0]] * 3 + [[1]] + [[0]] * 6
        beta[[3, 6, 8, 9], :2] = 0
    beta = torch.from_numpy(beta.astype(np.float32)).cuda()
    R = torch.from_numpy(rng.rand(K, 3) * (np.array(sz) - 1)).cuda()
    frames = torch.rand(T, nchan * P, device="cuda")
    tracks = ops.invert_quadratic_warp(beta, R)
    assert bool(torch.isfinite(tracks).all())
    tracks32 = tracks.float()
    print(f"{name}: K = {K}, T = {T}, {sz[0]}x{sz[1]}x{sz[2]}, rows of {nchan} channel(s)")
    for label, fn in (("K11 fit_quadratic_warp (quadratic, fp64 tracks)", lambda: ops.fit_quadratic_warp(tracks, R, sz)),
                      ("K11 fit_quadratic_warp (quadratic, fp32 tracks)", lambda: ops.fit_quadratic_warp(tracks32, R, sz)),
                      ("K11 fit_quadratic_warp (affine, fp32 tracks)", lambda: ops.fit_quadratic_warp(tracks32, R, sz, order="affine")),
                      ("K12 invert_quadratic_warp", lambda: ops.invert_quadratic_warp(beta, R)),
                      ("K13 roi_signals, window (3, 3, 0)", lambda: ops.roi_signals(frames, sz, tracks32, (3, 3, 0))),
                      ("K13 roi_signals, window (7, 7, 0)", lambda: ops.roi_signals(frames, sz, tracks32, (7, 7, 0)))):
        t = timed(fn, repeats)
        print(f"  {label}: {t * 1e3:.3f} ms per call, {t * 1e6 / T:.3f} us per frame (wrapper included)", flush=True)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    case("bench volume", [512, 512, 1], 100, 4000, 1, repeats)
    case("multi-channel rows", [512, 512, 1], 200, 1000, 3, repeats)


if __name__ == "__main__":
    main()
