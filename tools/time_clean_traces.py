#!/usr/bin/env python3
"""Time K20 (the trace clean-up, dnmf_clean_traces) with HIP events around the whole call, beside two compositions in the same run:
python tools/time_clean_traces.py [repeats] [--quick]

K = 100 traces of T = 4000 frames and K = 200 of T = 16 000, at fps = 4 and fps = 30 (running medians over W = 40 / 300 frames),
detrend modes 2 and 3.  Beside each: the float64 numpy restatement (tests/traces_restatement.py) on the CPU, timed on the first
NCPU traces and scaled to K (it loops over the traces; mode 3 couples them only through one median of K numbers), and a torch
composition of the running median alone on the GPU -- NaN padding, ``unfold`` and ``nanmedian`` over the window, float64, eight
traces at a time (torch's nanmedian takes the lower of two middle values where K20 takes their mean).  Also prints the largest
difference between K20's traces and the restatement's on those NCPU traces (mode 2).  ``--quick``: K = 8, T = 1000 (a rehearsal of
the script, not a measurement)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dnmf_amd import ops  # noqa: E402
import traces_restatement as TR  # noqa: E402

NCPU = 4


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


def make(K, T, seed=0):
    rng = np.random.RandomState(seed)
    t = np.arange(T)
    tau = rng.uniform(0.3, 3.0, K) * T
    x = (20.0 + 3.0 * rng.rand(K, T)) * np.exp(-t[None, :] / tau[:, None])
    x[rng.rand(K, T) < 0.02] = 0.0
    return x.astype(np.float32)


def torch_running_median(x, W):
    h = W // 2
    out = torch.empty_like(x)
    for s in range(0, x.shape[0], 8):
        pad = torch.nn.functional.pad(x[s:s + 8], (h, W - 1 - h), value=float("nan"))
        out[s:s + 8] = pad.unfold(1, W, 1).nanmedian(dim=2).values
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 3
    quick = "--quick" in sys.argv
    for K, T in ((100, 4000), (200, 16000)):
        if quick:
            K, T = 8, 1000
        x = make(K, T)
        xd = torch.from_numpy(x).cuda()
        ws = None
        for fps in (4.0, 30.0):
            W = TR.mround(10 * fps)
            for mode in (2, 3):
                out = ops.clean_traces(xd, fps, detrend_mode=mode, workspace=ws)
                ws = out[3]["workspace"]
                tk = best(lambda: ops.clean_traces(xd, fps, detrend_mode=mode, workspace=ws), repeats)
                t0 = time.perf_counter()
                ref = TR.clean_traces(x[:NCPU], fps, detrend_mode=mode)
                tc = (time.perf_counter() - t0) / NCPU * K * 1e3
                line = f"K={K} T={T} fps={fps:g} (W={W}) mode {mode}: K20 {tk:.3f} ms; numpy restatement {tc:.0f} ms ({NCPU} traces scaled to {K})"
                if mode == 2:
                    got = out[0][:NCPU].cpu().numpy().astype(np.float64)
                    same = np.array_equal(np.isnan(got), np.isnan(ref[0]))
                    line += f"; same NaNs {same}, largest difference of the traces {np.nanmax(np.abs(got - ref[0])):.2e}"
                print(line, flush=True)
            xm = torch.where(xd > 0.01, xd, torch.full_like(xd, float("nan"))).double()
            tt = best(lambda: torch_running_median(xm, W), min(repeats, 2))
            print(f"K={K} T={T} fps={fps:g} (W={W}): torch unfold + nanmedian, the running median alone, float64: {tt:.3f} ms", flush=True)
            del xm
        if quick:
            break


if __name__ == "__main__":
    main()
