#!/usr/bin/env python3
"""Time K26 (dnmf_component_pairs, dnmf_merge_apply) with HIP events around the whole ``ops`` calls, beside a torch composition in
the same run:
python tools/time_merge.py [repeats] [--quick]

K = 100 Gaussian footprints (sigma 3) at random centres in 512x512x1 with T = 4000 frames, and K = 200 in 512x512x2 with T = 1000;
every tenth centre has a twin one voxel away whose trace is a share of the same trace plus noise, so that there is something to
merge.  ``component_pairs`` is timed on its default pairs (the diagonal and the i < j whose boxes intersect) with the boxes and the
pairs already made -- the call still checks them on the host and copies them to the device -- and ``merge_apply`` on the plan of those
statistics.  The composition, in fp32 on the GPU: ``A_rows @ A_rows.T``, every pair over the whole volume whether or not the boxes
meet, and ``torch.corrcoef(C)``; it has no NaN handling and no shifted sums.  A timed window is as many calls between two events as
take about 50 ms (at most INNER); the best of ``repeats`` windows is printed.  ``--quick``: K = 12, T = 200, 64x64 (a rehearsal of
the script, not a measurement)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dnmf_amd import ops  # noqa: E402

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


def make(K, T, sz, seed):
    rng = np.random.RandomState(seed)
    X, Y, Z = sz
    pos = np.stack([rng.uniform(8, X - 8, K), rng.uniform(8, Y - 8, K), np.full(K, 0.5 * (Z - 1))], 1)
    C = rng.gamma(2.0, 1.0, (K, T))
    for k in range(0, K - 1, 10):                                     # k + 1 is the twin of k
        pos[k + 1] = pos[k] + [1.0, 0.0, 0.0]
        share = rng.uniform(0.3, 0.7)
        C[k + 1] = (1 - share) * C[k] * (1 + 0.05 * rng.randn(T))
        C[k] = share * C[k] * (1 + 0.05 * rng.randn(T))
    A = torch.zeros((X * Y * Z, K), dtype=torch.float32, device="cuda")
    gx, gy, gz = torch.meshgrid(torch.arange(X), torch.arange(Y), torch.arange(Z), indexing="ij")
    grid = torch.stack((gx, gy, gz), 3).reshape(-1, 3).float().cuda()
    for k in range(K):
        A[:, k] = torch.exp(-((grid - torch.tensor(pos[k], dtype=torch.float32, device="cuda")) ** 2).sum(1) / 9.0)
    return A, torch.from_numpy(np.maximum(C, 0.0).astype(np.float32)).cuda()


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    quick = "--quick" in sys.argv
    for K, T, sz in ((100, 4000, (512, 512, 1)), (200, 1000, (512, 512, 2))):
        if quick:
            K, T, sz = 12, 200, (64, 64, 1)
        A, C = make(K, T, sz, 0)
        A_rows = A.t().contiguous()
        boxes = ops.component_boxes(A, sz, floor=1e-3, margin=0).cpu()
        pairs = ops.candidate_pairs(boxes)
        stats = ops.component_pairs(A_rows, sz, boxes, C, pairs=pairs)
        groups = ops.merge_groups(stats, K, 0.85, 0.1)
        gstats = ops.component_pairs(A_rows, sz, boxes, C, pairs=ops.merge_group_pairs(groups))
        plan = ops.merge_plan(stats, K, 0.85, 0.1, group_stats=gstats)
        A_out = torch.empty((A.shape[0], len(groups)), dtype=torch.float32, device="cuda")
        C_out = torch.empty((len(groups), T), dtype=torch.float32, device="cuda")
        # the composition's answers against the kernel's, where both are defined
        gram, cc = A_rows @ A_rows.t(), torch.corrcoef(C)
        pl = stats["pairs"].long()
        off = pl[:, 0] != pl[:, 1]
        dc = float((cc[pl[off, 0], pl[off, 1]].double() - stats["corr"][off]).abs().max()) if bool(off.any()) else 0.0
        timed = [best(lambda: ops.component_pairs(A_rows, sz, boxes, C, pairs=pairs), repeats),
                 best(lambda: ops.merge_apply(A, C, plan, A_out=A_out, C_out=C_out), repeats),
                 best(lambda: (A_rows @ A_rows.t(), torch.corrcoef(C)), repeats)]
        how = ["%.3f ms (best of %d windows of %d calls)" % (t, w, n) for t, n, w in timed]
        print(f"K={K} T={T} {sz[0]}x{sz[1]}x{sz[2]}: {len(pairs)} pairs, {plan['merged']} groups merged, K' = {len(groups)}; "
              f"component_pairs {how[0]}; merge_apply {how[1]}; torch A_rows @ A_rows.T + corrcoef in fp32 {how[2]}; largest "
              f"difference of corr from torch.corrcoef {dc:.1e}; gram {tuple(gram.shape)}", flush=True)
        if quick:
            break


if __name__ == "__main__":
    main()
