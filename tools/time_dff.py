#!/usr/bin/env python3
"""Time K31 (dnmf_running_quantile, dnmf_baseline_apply: the running-percentile baseline and the dF/F movie) with HIP events
around the whole ``ops`` calls, beside each kernel's traffic floor and beside the composition a user would write, in the same run:
python tools/time_dff.py [repeats] [--quick]

512x512x1 with 4000 frames and 512x512x2 with 1000, each with (window, stride) = (400, 100) and (1200, 300) at the 8th
percentile, and 100 traces of 4000 frames with window 400 and stride 1 (an exact running percentile filter).  Prints per case
* ``ops.running_quantile`` and ``ops.baseline_apply`` (mode 'dff'), best of ``repeats`` after a warm-up, each with its share of its
  floor -- 4 B (K31a: every sample read once) and 8 B (K31b: read and written) per voxel and frame at the device-copy bandwidth
  measured in this run (a copy reads and writes: its bytes are counted twice);
* the torch composition: per knot ``torch.nanquantile`` of the window's slice (``unfold`` for stride 1), then the two bracketing
  knots of every frame and a ``lerp``, with the largest difference between its dF/F and K31's.
``--quick``: 64 x 64 voxels (a rehearsal of the script, not a measurement)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402

SLAB = 1 << 23


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


def copy_bandwidth(frames, repeats):
    """Bytes per second of a device copy of the movie (read + write)."""
    out = torch.empty_like(frames)
    t = best(lambda: out.copy_(frames), repeats)
    return 2.0 * frames.numel() * 4 / (t * 1e-3)


def torch_dff(frames, plan, q):
    """The composition: knots by nanquantile per window, then the bracketing knots of every frame and a lerp -> (T, P) fp32."""
    T, P = frames.shape
    starts, ends = plan["starts"], plan["ends"]
    W = int(ends[0] - starts[0])
    # torch.quantile takes a bounded number of elements a call: the windows go in slabs of SLAB elements
    if len(starts) > 1 and int(starts[1] - starts[0]) == 1:
        windows, step = frames.t().unfold(1, W, 1), max(1, SLAB // (W * P))                       # (P, J, W)
        knots = torch.cat([torch.nanquantile(windows[:, a:a + step], q, dim=2) for a in range(0, windows.shape[1], step)], 1).t().contiguous()
    else:
        step = max(1, SLAB // W)
        knots = torch.stack([torch.cat([torch.nanquantile(frames[int(s):int(e), a:a + step], q, dim=0) for a in range(0, P, step)])
                             for s, e in zip(starts, ends)])
    c = torch.as_tensor(plan["centres"], device=frames.device)
    t = torch.arange(T, device=frames.device, dtype=torch.float64)
    j = (torch.searchsorted(c, t, right=True) - 1).clamp(0, len(c) - 1)
    j2 = (j + 1).clamp(max=len(c) - 1)
    w = ((t - c[j]) / (c[j2] - c[j]).clamp(min=1.0)).clamp(0.0, 1.0).float()[:, None]
    f0 = torch.lerp(knots[j], knots[j2], w)
    return (frames - f0) / f0


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 3
    quick = "--quick" in sys.argv
    cases = [([512, 512, 1], 4000, 400, 100), ([512, 512, 1], 4000, 1200, 300), ([512, 512, 2], 1000, 400, 100),
             ([512, 512, 2], 1000, 1200, 300), ([100, 1, 1], 4000, 400, 1)]
    for sz, T, W, S in cases:
        if quick and sz[1] > 1:
            sz = [64, 64, sz[2]]
        P = sz[0] * sz[1] * sz[2]
        name = f"{sz[0]}x{sz[1]}x{sz[2]} x {T} frames, window {W}, stride {S}"
        torch.manual_seed(0)
        decay = torch.exp(-torch.arange(T, device="cuda") / (2.0 * T))[:, None]
        frames = (1.0 + torch.rand(T, P, device="cuda")) * decay + (torch.rand(T, P, device="cuda") < 0.02) * 3.0
        big = frames if P * T >= 1 << 24 else torch.rand(1 << 26, device="cuda")
        bw = copy_bandwidth(big, repeats)
        floor_a, floor_b = 4.0 * P * T / bw * 1e3, 8.0 * P * T / bw * 1e3
        print(f"{name}: device copy {bw / 1e12:.2f} TB/s; floors {floor_a:.3f} ms (K31a, 4 B) and {floor_b:.3f} ms (K31b, 8 B)", flush=True)
        plan = ops.running_window_plan(T, W, S)
        ta = best(lambda: ops.running_quantile(frames, sz, W, S, 0.08), repeats)
        knots = ops.running_quantile(frames, sz, W, S, 0.08)
        out = torch.empty_like(frames)
        tb = best(lambda: ops.baseline_apply(frames, sz, knots["value"], knots["centres"], "dff", out=out), repeats)
        print(f"{name}: running_quantile ({plan['J']} windows) {ta:.3f} ms ({floor_a / ta:.3f} of its floor); baseline_apply {tb:.3f} ms "
              f"({floor_b / tb:.2f} of its floor)", flush=True)
        tt = best(lambda: torch_dff(frames, plan, 0.08), min(repeats, 1))
        ref = torch_dff(frames, plan, 0.08)
        print(f"{name}: torch nanquantile per knot + lerp {tt:.3f} ms; largest difference between its dF/F and K31's "
              f"{float((ref - out).abs().max()):.2e}", flush=True)
        del frames, out, ref, big


if __name__ == "__main__":
    main()
