#!/usr/bin/env python3
"""Time K24 (dnmf_component_stats: per-component sums, frame correlations, raw traces, mean images and r_values) with HIP
events, beside a torch composition of the same outputs, in the same run:
python tools/time_components.py [repeats] [--quick]

K = 100 at 512x512x1 with 4000 frames and K = 200 at 512x512x2 with 1000; Gaussian footprints of sigma 3 at random centres,
boxes from ``ops.component_boxes`` (about 21 x 21 x Z voxels), a quarter of the frames weighted; with and without ``sub``.
The whole ``ops.component_stats`` call is timed (both launches, the allocation of the outputs, the host's look at the
boxes), the state reused.  Prints per case the best time and its share of the floor sum_k B n_k 8 bytes (4 without ``sub``)
at the copy bandwidth measured in the same run.  That floor counts only the box samples: neighbouring boxes overlap and a
box's rows are short runs of full cache lines, so most of these reads are served from cache and HBM sees other traffic -- a
share above 1 is possible, and the figure is a yardstick for the kernel's own progress, not a roofline.
The torch composition is what a user without the kernel would chain, in fp32: index the boxes of a piece of frames
(advanced indexing with a padded (K, vmax) index table and a mask), form e, then ``bmm`` for sum a e and for the weighted
image, elementwise sums for the rest, pieces sized to 1 GiB of gathered samples; no handling of samples that are not
finite.  The largest difference between its outputs and K24's is printed.  ``--quick``: 64 frames (a rehearsal of the
script, not a measurement)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402


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


def footprints(sz, K):
    """(P, K) fp32: exp(-|u - centre_k|^2 / 9) at random centres."""
    X, Y, Z = sz
    g = torch.stack(torch.meshgrid(torch.arange(X), torch.arange(Y), torch.arange(Z), indexing="ij"), -1).reshape(-1, 3).float().cuda()
    centres = torch.rand(K, 3, device="cuda") * torch.tensor([X - 1, Y - 1, Z - 1], device="cuda")
    A = torch.empty((X * Y * Z, K), device="cuda")
    for k in range(K):
        A[:, k] = torch.exp(-((g - centres[k]) ** 2).sum(1) / 9.0)
    return A


def box_table(boxes, sz):
    """(K, vmax) voxel indices of the boxes, x slowest, padded with 0; the mask of the real entries."""
    Y, Z = sz[1], sz[2]
    b = boxes.cpu().long()
    ext = b[:, 1::2] - b[:, 0::2] + 1
    n = ext.prod(1)
    vmax = int(n.max())
    idx = torch.zeros((b.shape[0], vmax), dtype=torch.long)
    for k in range(b.shape[0]):
        x, y, z = torch.meshgrid(*[torch.arange(int(b[k, 2 * d]), int(b[k, 2 * d + 1]) + 1) for d in range(3)], indexing="ij")
        idx[k, :int(n[k])] = ((x * Y + y) * Z + z).reshape(-1)
    mask = torch.arange(vmax)[None, :] < n[:, None]
    return idx.cuda(), mask.cuda(), n.cuda()


def pearson(n, sa, saa, sb, sbb, sab):
    return (n * sab - sa * sb) / ((n * saa - sa * sa) * (n * sbb - sb * sb)).sqrt()


def torch_stats(frames, sub, A_rows, idx, mask, n, C, w, piece):
    """The outputs of K24 from gathers and ``bmm``, fp32: sums (K, B, 3), frame_corr, raw (K, B), image (K, vmax), r_values."""
    K, vmax = idx.shape
    B = frames.shape[0]
    m = mask.float()
    a = A_rows.gather(1, idx) * m                                        # (K, vmax)
    nf = n.float()
    sa, saa = a.sum(1), (a * a).sum(1)
    sums = torch.empty((K, B, 3), device=frames.device)
    img = torch.zeros((K, vmax), device=frames.device)
    for s in range(0, B, piece):
        E = frames[s:s + piece][:, idx]                                 # (b, K, vmax)
        if sub is not None:
            E = E - sub[s:s + piece][:, idx]
        E = (E.permute(1, 0, 2) + a[:, None, :] * C[:, s:s + piece, None]) * m[:, None, :]      # (K, b, vmax)
        sums[:, s:s + piece, 0] = E.sum(2)
        sums[:, s:s + piece, 1] = (E * E).sum(2)
        sums[:, s:s + piece, 2] = torch.bmm(E, a[:, :, None])[:, :, 0]
        img += torch.bmm(w[:, None, s:s + piece], E)[:, 0]
    se, see, sae = sums.unbind(2)
    corr = pearson(nf[:, None], sa[:, None], saa[:, None], se, see, sae)
    raw = (nf[:, None] * sae - sa[:, None] * se) / (nf * saa - sa * sa)[:, None]
    image = img / w.sum(1, keepdim=True)
    r = pearson(nf, sa, saa, (image * m).sum(1), (image * image * m).sum(1), (a * image).sum(1))
    return sums, corr, raw, image, r


def copy_bandwidth(t):
    """Bytes per second of a device copy of ``t`` (read plus write), best of 5."""
    out = torch.empty_like(t)
    ms = best(lambda: out.copy_(t), 5)
    return 2.0 * t.numel() * t.element_size() / (ms * 1e-3)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    quick = "--quick" in sys.argv
    for sz, T, K in (([512, 512, 1], 4000, 100), ([512, 512, 2], 1000, 200)):
        if quick:
            T = 64
        P = sz[0] * sz[1] * sz[2]
        torch.manual_seed(0)
        frames = 1.0 + torch.rand(T, P, device="cuda")
        sub = torch.rand(T, P, device="cuda")
        bw = copy_bandwidth(frames)
        A = footprints(sz, K)
        A_rows = A.t().contiguous()
        boxes = ops.component_boxes(A, sz)
        idx, mask, n = box_table(boxes, sz)
        del A
        C = torch.rand(K, T, device="cuda")
        w = (torch.rand(K, T, device="cuda") < 0.25).float()
        name = f"{sz[0]}x{sz[1]}x{sz[2]} x {T} frames, K = {K}, boxes of {int(n.min())}..{int(n.max())} voxels"
        print(f"{name}: device copy {bw / 1e12:.2f} TB/s", flush=True)
        state = None
        for with_sub in (False, True):
            s = sub if with_sub else None
            _, state = ops.component_stats(frames, sz, A_rows, boxes, C, w, sub=s, state=state)
            t = best(lambda: ops.component_stats(frames, sz, A_rows, boxes, C, w, sub=s, state=state), repeats)
            floor_ms = (8.0 if with_sub else 4.0) * float(n.sum()) * T / bw * 1e3
            print(f"{name}{', sub' if with_sub else ''}: K24 {t:.3f} ms ({floor_ms / t:.2f} of the floor of {floor_ms:.3f} ms: box samples "
                  f"at the copy bandwidth, reads served mostly from cache)", flush=True)
            piece = max(1, (1 << 30) // (4 * idx.numel()))
            tt = best(lambda: torch_stats(frames, s, A_rows, idx, mask, n, C, w, piece), min(repeats, 2))
            out, _ = ops.component_stats(frames, sz, A_rows, boxes, C, w, sub=s, state=state)
            ref = torch_stats(frames, s, A_rows, idx, mask, n, C, w, piece)
            image = torch.where(mask, out["image"], torch.zeros((), dtype=torch.float64, device="cuda"))
            rel = float(((out["sums"] - ref[0].double()).abs() / out["sums"].abs().clamp_min(1.0)).max())
            dev = max(float((got - r.double()).abs().max()) for got, r in
                      zip((out["frame_corr"], out["raw"], image, out["r_values"]), (ref[1], ref[2], ref[3] * mask, ref[4])))
            print(f"{name}{', sub' if with_sub else ''}: torch composition (fp32, pieces of {piece} frames) {tt:.3f} ms, {tt / t:.1f} times "
                  f"K24; largest difference of its sums {rel:.2e} relative, of frame_corr / raw / image / r_values {dev:.2e}", flush=True)
        del frames, sub, state


if __name__ == "__main__":
    main()
