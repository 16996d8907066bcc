#!/usr/bin/env python3
"""Time K28 (dnmf_residual_boxes, dnmf_rank1_nmf) with HIP events around the whole ``ops`` calls, beside a torch composition in the
same run:
python tools/time_add.py [repeats] [--quick]

M = 20 candidate boxes of 13 x 13 x 1 voxels at random centres in 512x512x1 with T = 4000 frames, and M = 40 boxes of 13 x 13 x 2 in
512x512x2 with T = 1000; the frames are noise plus one Gaussian cell per box with a gamma trace, ``sub`` is a second buffer of the
same size.  ``residual_boxes`` is timed with the boxes already made -- the call still checks them on the host and copies them to the
device -- and ``rank1_nmf`` with five rounds on its result.  The composition, in fp32 on the GPU: ``(frames - sub).index_select(1,
voxels)`` for the gather (it subtracts the whole movie first, and takes boxes of one size only), and five rounds of ``bmm`` with
clamps for the factor; it has no NaN handling and no float64.  A timed window is as many calls between two events as take about
50 ms (at most INNER); the best of ``repeats`` windows is printed.  ``--quick``: M = 3, T = 100, 64x64 (a rehearsal of the script,
not a measurement)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dnmf_amd import ops  # noqa: E402

INNER = 500
ITERS = 5


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


def torch_gather(frames, sub, vox):
    M, n = vox.shape
    return (frames - sub).index_select(1, vox.reshape(-1)).reshape(-1, M, n).permute(1, 0, 2).contiguous()


def torch_factor(E, a0):
    a = a0.clone()
    for it in range(ITERS + 1):
        if it == ITERS:
            a = a * (a0.norm(dim=1, keepdim=True) / a.norm(dim=1, keepdim=True))
        c = torch.bmm(E, a[:, :, None])[:, :, 0].clamp_min(0) / (a * a).sum(1, keepdim=True)
        if it < ITERS:
            a = torch.bmm(c[:, None, :], E)[:, 0, :].clamp_min(0) / (c * c).sum(1, keepdim=True)
    return a, c


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    quick = "--quick" in sys.argv
    for M, T, sz in ((20, 4000, (512, 512, 1)), (40, 1000, (512, 512, 2))):
        if quick:
            M, T, sz = 3, 100, (64, 64, 1)
        X, Y, Z = sz
        P = X * Y * Z
        rng = np.random.RandomState(0)
        centres = np.stack([rng.uniform(8, X - 8, M), rng.uniform(8, Y - 8, M), np.full(M, 0.5 * (Z - 1))], 1)
        boxes = ops.candidate_boxes(torch.from_numpy(centres), sz, [6, 6, 0 if Z == 1 else 1])
        nvox = (boxes[:, 1::2] - boxes[:, 0::2] + 1).long().prod(1)
        assert int(nvox.min()) == int(nvox.max())          # the composition takes boxes of one size
        vmax = int(nvox.max())
        gen = torch.Generator(device="cuda").manual_seed(0)
        frames = 0.1 * torch.randn((T, P), device="cuda", generator=gen)
        sub = 0.1 * torch.randn((T, P), device="cuda", generator=gen)
        b = boxes.long()
        g = [torch.arange(int(b[0, 2 * d + 1] - b[0, 2 * d]) + 1) for d in range(3)]
        rel = torch.stack(torch.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3)
        vox = (((b[:, None, 0] + rel[None, :, 0]) * Y + b[:, None, 2] + rel[None, :, 1]) * Z + b[:, None, 4] + rel[None, :, 2]).cuda()
        a0 = torch.exp(-((rel[None].double() + b[:, None, 0::2].double() - torch.from_numpy(centres)[:, None, :]) ** 2).sum(2) / 9.0)
        a0 = a0.float().cuda().contiguous()
        traces = torch.from_numpy(rng.gamma(2.0, 1.0, (M, T)).astype(np.float32)).cuda()
        for m in range(M):
            frames[:, vox[m]] += traces[m][:, None] * a0[m][None, :]
        E = ops.residual_boxes(frames, sz, boxes, sub=sub)
        fit = ops.rank1_nmf(E, nvox, a0, iters=ITERS)
        Et = torch_gather(frames, sub, vox)
        at, ct = torch_factor(Et, a0)
        same = bool(torch.equal(E, Et))
        da = float((fit["a"] - at).abs().max() / at.abs().max())
        ws = torch.empty(M * T * 2 + 64, dtype=torch.float32, device="cuda")
        timed = [best(lambda: ops.residual_boxes(frames, sz, boxes, sub=sub, out=E), repeats),
                 best(lambda: ops.rank1_nmf(E, nvox, a0, iters=ITERS, workspace=ws), repeats),
                 best(lambda: torch_gather(frames, sub, vox), repeats),
                 best(lambda: torch_factor(Et, a0), repeats)]
        how = ["%.3f ms (best of %d windows of %d calls)" % (t, w, n) for t, n, w in timed]
        print(f"M={M} T={T} {X}x{Y}x{Z}, boxes of {vmax} voxels: residual_boxes {how[0]}; rank1_nmf, {ITERS} rounds {how[1]}; torch "
              f"(frames - sub).index_select {how[2]}; torch bmm rounds in fp32 {how[3]}; gather equal to torch's bit for bit: {same}; "
              f"largest difference of a from the fp32 composition {da:.1e} of its maximum; all ok: {bool(fit['ok'].all())}", flush=True)
        if quick:
            break


if __name__ == "__main__":
    main()
