#!/usr/bin/env python3
"""Time K18 (dnmf_summary_images: mean, std, max and the local correlation image of a video) with HIP events, beside the
same four images from a torch composition, in the same run:
python tools/time_summary.py [repeats] [--quick]

512x512x1 with 4000 frames and 512x512x2 with 1000; 'full' and 'face' neighbourhoods, with and without ``sub``.  Prints per
case the best time of K18 and its share of the HBM floor: 4 bytes per voxel and frame (8 with ``sub``) at the 8 TB/s roof.
The torch composition works in fp32 (mean, var, amax over time, then one product of shifted views and a sum per direction
of the half-set, no handling of voxels that are not finite): what a user without the kernel would chain; it is timed once
per size and neighbourhood, on the plain frames.  ``--quick``: 64 frames (a rehearsal of the script, not a measurement)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402

HBM_ROOF = 8.0e12   # bytes / s


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


def half_set(neighbours, sz):
    out = []
    for dx in (0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                d = (dx, dy, dz)
                if d <= (0, 0, 0) or (neighbours == "face" and sum(abs(v) for v in d) != 1):
                    continue
                if all(v == 0 or s > 1 for v, s in zip(d, sz)):
                    out.append(d)
    return out


def cut(n, d):
    """The slices of an axis of n voxels for a voxel and for its neighbour at +d."""
    return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))


def torch_images(video, neighbours):
    """video (T, X, Y, Z) fp32 -> mean, std, max, corr (X, Y, Z) fp32."""
    T, sz = video.shape[0], tuple(video.shape[1:])
    mean = video.mean(0)
    var = video.var(0, unbiased=False)
    mx = video.amax(0)
    c = video - mean
    sd = var.sqrt()
    acc = torch.zeros_like(mean)
    cnt = torch.zeros_like(mean)
    for d in half_set(neighbours, sz):
        (ax, bx), (ay, by), (az, bz) = (cut(n, v) for n, v in zip(sz, d))
        r = (c[:, ax, ay, az] * c[:, bx, by, bz]).sum(0) / T / (sd[ax, ay, az] * sd[bx, by, bz])
        acc[ax, ay, az] += r
        acc[bx, by, bz] += r
        cnt[ax, ay, az] += 1
        cnt[bx, by, bz] += 1
    return mean, sd, mx, acc / cnt


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    quick = "--quick" in sys.argv
    for sz, T in (([512, 512, 1], 4000), ([512, 512, 2], 1000)):
        if quick:
            T = 64
        P = sz[0] * sz[1] * sz[2]
        torch.manual_seed(0)
        frames = 1.0 + torch.rand(T, P, device="cuda")
        sub = torch.rand(T, P, device="cuda")
        for neighbours in ("full", "face"):
            state = ops.summary_images_state(sz, T, neighbours=neighbours)
            for with_sub in (False, True):
                t = best(lambda: ops.summary_images(frames, sz, sub=sub if with_sub else None, neighbours=neighbours, state=state), repeats)
                floor_ms = (8.0 if with_sub else 4.0) * P * T / HBM_ROOF * 1e3
                print(f"{sz[0]}x{sz[1]}x{sz[2]} x {T} frames, {neighbours}{', sub' if with_sub else ''}: K18 {t:.3f} ms "
                      f"({floor_ms / t:.2f} of the HBM floor of {floor_ms:.3f} ms)", flush=True)
            video = frames.view(T, *sz)
            tt = best(lambda: torch_images(video, neighbours), min(repeats, 2))
            images, _ = ops.summary_images(frames, sz, neighbours=neighbours, state=state)
            ref = torch_images(video, neighbours)
            dev = max(float((images[k] - r.double()).abs().max()) for k, r in zip(("mean", "std", "max", "corr"), ref))
            print(f"{sz[0]}x{sz[1]}x{sz[2]} x {T} frames, {neighbours}: torch composition (fp32) {tt:.3f} ms; largest difference "
                  f"between its images and K18's {dev:.2e}", flush=True)
            del state
        del frames, sub


if __name__ == "__main__":
    main()
