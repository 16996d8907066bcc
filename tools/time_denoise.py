#!/usr/bin/env python3
"""Time K34 (dnmf_lowrank_*: local low-rank denoising of a movie) with HIP events around the whole ``ops`` calls, beside the
traffic floor and beside the composition a user would write, in the same run:
python tools/time_denoise.py [repeats] [--quick]

512x512x1 with 4000 frames and 512x512x2 with 1000, patch (16, 16, None), overlap (8, 8, 0), R = 8.  Prints per case
* each of the five pieces -- ``lowrank_accumulate``, ``lowrank_orthonormalise``, ``lowrank_project``, ``lowrank_ritz``,
  ``lowrank_reconstruct`` -- best of ``repeats`` after a warm-up, and the total of ``lowrank_denoise`` with ``iters = 4``; the movie
  is unit noise, of which ``keep='auto'`` keeps nothing, so the last two and the total are also timed with ``keep=8``;
* the floor of a pass: one read of the overlapping patches, 4 B x NP x n x T, at the device-copy bandwidth measured in this run
  (a copy reads and writes: its bytes are counted twice);
* the torch composition on a slab of patches -- ``unfold`` + ``torch.svd_lowrank(q=8, niter=4)`` -- scaled to all patches.
``--quick``: 64 x 64 voxels and 200 frames (a rehearsal of the script, not a measurement)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402

SLAB_PATCHES = 256


def best(fn, repeats, before=None):
    """The best of ``repeats`` timings of ``fn`` after a warm-up; ``before`` runs untimed ahead of every call."""
    times = []
    for _ in range(repeats + 1):                    # the first call warms up
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return min(times[1:])


def copy_bandwidth(frames, repeats):
    out = torch.empty_like(frames)
    t = best(lambda: out.copy_(frames), repeats)
    return 2.0 * frames.numel() * 4 / (t * 1e-3)


def torch_slab(frames, sz, npatch):
    """unfold + svd_lowrank on the first ``npatch`` 16 x 16 patches of plane z = 0 (stride 8)."""
    T = frames.shape[0]
    vol = frames.view(T, sz[0], sz[1], sz[2])[..., 0]
    patches = vol.unfold(1, 16, 8).unfold(2, 16, 8).reshape(T, -1, 256)[:, :npatch]          # (T, np, 256): materialised
    D = patches.permute(1, 2, 0).contiguous()
    D = D - D.mean(2, keepdim=True)
    U, S, V = torch.svd_lowrank(D, q=8, niter=4)
    return (U * S[:, None, :]) @ V.transpose(1, 2)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 2
    quick = "--quick" in sys.argv
    for sz, T in (([512, 512, 1], 4000), ([512, 512, 2], 1000)):
        if quick:
            sz, T = [64, 64, sz[2]], 200
        P = sz[0] * sz[1] * sz[2]
        name = f"{sz[0]}x{sz[1]}x{sz[2]} x {T} frames"
        torch.manual_seed(0)
        frames = 10.0 + torch.randn(T, P, device="cuda")
        bw = copy_bandwidth(frames if P * T >= 1 << 24 else torch.rand(1 << 26, device="cuda"), repeats)
        plan = ops.lowrank_patch_plan(sz)
        NP, n = len(plan["boxes"]), plan["n"]
        floor = 4.0 * NP * n * T / bw * 1e3
        print(f"{name}: {NP} patches of {n} voxels; device copy {bw / 1e12:.2f} TB/s; floor of a pass {floor:.3f} ms", flush=True)
        centre = frames.double().mean(0)
        state = ops.lowrank_state(plan, 8, T)
        out = torch.empty_like(frames)
        ta = best(lambda: ops.lowrank_accumulate(frames, sz, plan, state, centre), repeats)
        # K34b leaves W = 0: every timed call gets the W of a pass first, or it would orthonormalise nothing
        tb = best(lambda: ops.lowrank_orthonormalise(state), repeats, before=lambda: ops.lowrank_accumulate(frames, sz, plan, state, centre))
        tc = best(lambda: ops.lowrank_project(frames, sz, plan, state, centre), repeats)
        td = best(lambda: ops.lowrank_ritz(state), repeats)
        te = best(lambda: ops.lowrank_reconstruct(frames, sz, plan, state, centre, out=out), repeats)
        print(f"{name}: accumulate {ta:.3f} ms ({floor / ta:.3f} of the floor); orthonormalise {tb:.3f} ms; project {tc:.3f} ms "
              f"({floor / tc:.3f}); ritz {td:.3f} ms; reconstruct {te:.3f} ms", flush=True)
        td8 = best(lambda: ops.lowrank_ritz(state, keep=8), repeats)
        assert int(state["kept"].min()) == 8, "keep=8 must use every column of every patch"
        te8 = best(lambda: ops.lowrank_reconstruct(frames, sz, plan, state, centre, out=out), repeats)
        print(f"{name}: with keep=8 (every column used, what a movie with structure costs at most): ritz {td8:.3f} ms; reconstruct "
              f"{te8:.3f} ms", flush=True)
        del state
        tt = best(lambda: ops.lowrank_denoise(frames, sz, centre, out=out), min(repeats, 1))
        tt8 = best(lambda: ops.lowrank_denoise(frames, sz, centre, keep=8, out=out), min(repeats, 1))
        print(f"{name}: lowrank_denoise, iters = 4, R = 8: {tt:.3f} ms in all with keep='auto' (nothing kept), {tt8:.3f} ms with keep=8",
              flush=True)
        slab = min(SLAB_PATCHES, ((sz[0] - 16) // 8 + 1) * ((sz[1] - 16) // 8 + 1))
        ts = best(lambda: torch_slab(frames, sz, slab), min(repeats, 1))
        print(f"{name}: torch unfold + svd_lowrank(q=8, niter=4) on {slab} patches of plane 0: {ts:.3f} ms, x {NP / slab:.1f} for {NP} "
              f"patches = {ts * NP / slab:.1f} ms (fp32, no blend)", flush=True)
        del frames, out


if __name__ == "__main__":
    main()
