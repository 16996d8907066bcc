#!/usr/bin/env python3
"""Time K30 (dnmf_temporal_select_*: exact per-voxel quantiles over time) with HIP events around the whole ``ops`` sequence,
beside its traffic floor and beside the composition a user would write, in the same run:
python tools/time_robust.py [repeats] [--quick]

512x512x1 with 4000 frames and 512x512x2 with 1000.  Prints per case
* ``ops.temporal_quantiles`` for q = 0.5 alone, for q = (0.5, 1) and for four quantiles, and ``ops.robust_images`` whole (three
  selections: values, |y - median|, |adjacent differences|), each with its share of the floor: passes x 4 bytes per voxel and
  frame at the device-copy bandwidth measured in this run (a copy reads and writes: its bytes are counted twice);
* ``torch.kthvalue`` and ``torch.quantile`` over dim 0, the composition a user would write: the movie in 8 slabs of voxels
  (the slab bounds the contiguous copy and the sort's workspace to an eighth of the movie each), timed over all slabs, with
  the largest difference between its median and K30's.
``--quick``: 64 frames (a rehearsal of the script, not a measurement)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402

SLABS = 8


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


def torch_median(frames, how):
    """The lower median (kthvalue) or the interpolated one (quantile) over dim 0, slab by slab -> (P,) fp32."""
    T, P = frames.shape
    out = torch.empty(P, device=frames.device)
    step = (P + SLABS - 1) // SLABS
    for s in range(0, P, step):
        slab = frames[:, s:s + step].contiguous()
        out[s:s + step] = torch.kthvalue(slab, (T + 1) // 2, dim=0).values if how == "kthvalue" else torch.quantile(slab, 0.5, dim=0)
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 3
    quick = "--quick" in sys.argv
    passes = ops.temporal_quantiles_passes()
    for sz, T in (([512, 512, 1], 4000), ([512, 512, 2], 1000)):
        if quick:
            T = 64
        P = sz[0] * sz[1] * sz[2]
        name = f"{sz[0]}x{sz[1]}x{sz[2]} x {T} frames"
        torch.manual_seed(0)
        frames = 1.0 + torch.rand(T, P, device="cuda") + (torch.rand(T, P, device="cuda") < 0.02) * 3.0
        bw = copy_bandwidth(frames, repeats)
        floor_ms = passes * 4.0 * P * T / bw * 1e3
        print(f"{name}: device copy {bw / 1e12:.2f} TB/s; the floor of one selection ({passes} passes x 4 B) {floor_ms:.3f} ms", flush=True)
        for q in ([0.5], [0.5, 1.0], [0.0, 0.08, 0.5, 1.0]):
            t = best(lambda: ops.temporal_quantiles(frames, sz, q), repeats)
            print(f"{name}: temporal_quantiles q={q}: {t:.3f} ms ({floor_ms / t:.2f} of the floor)", flush=True)
        t = best(lambda: ops.robust_images(frames, sz), repeats)
        print(f"{name}: robust_images (3 selections): {t:.3f} ms ({3 * floor_ms / t:.2f} of its floor of {3 * floor_ms:.3f} ms)", flush=True)
        mine = ops.temporal_quantiles(frames, sz, [0.5])[0]
        for how in ("kthvalue", "quantile"):
            tt = best(lambda: torch_median(frames, how), min(repeats, 2))
            ref = torch_median(frames, how).double()
            got = (mine["lo"][0] if how == "kthvalue" else mine["value"][0]).reshape(-1).double()
            print(f"{name}: torch.{how} over dim 0 in {SLABS} slabs: {tt:.3f} ms; largest difference between its median and K30's "
                  f"{float((got - ref).abs().max()):.2e}", flush=True)
        del frames


if __name__ == "__main__":
    main()
