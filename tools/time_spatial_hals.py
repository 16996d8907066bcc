#!/usr/bin/env python3
"""Time K6h (dnmf_hals_spatial_lists), the exact footprint solver, with HIP events around the whole ``ops`` calls, beside the
multiplicative update it stands next to:
python tools/time_spatial_hals.py [repeats] [--quick]

K = 100 Gaussian footprints (the model's, sigma 3) at random centres in 512x512x1 with T = 4000 registered frames, and K = 200
in 512x512x2 with T = 1000.  Timed: the list K5 once (the movie pass both solvers need), ``mu_spatial_lists`` once, K6h at 1, 5
and 20 sweeps (each call first restores the sums it overwrites: a copy of ``total`` floats, inside the window), then
``iter_a = 5`` full multiplicative ``spatial_step``s against ONE ``spatial_step(solver='hals', sweeps=5)``.  K6h's floor is
stated against 8 TB/s: the sums ``A1c`` read (4 ``total`` bytes), the rows of ``At`` read (4 ``total``) and the entries written
(4 ``total``); the scatter into ``A`` that both solvers share reads 4 ``total`` more and writes as many.  A timed window is as
many calls between two events as take about 50 ms (at most INNER); the best of ``repeats`` windows is printed.  ``--quick``:
K = 12, T = 200, 64x64 (a rehearsal of the script, not a measurement)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dnmf_amd import ops  # noqa: E402
from dnmf_amd.Demix import dNMF  # noqa: E402

INNER = 500
HBM_ROOF = 8.0e12   # bytes / s


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def best(fn, repeats):
    """ms per call: the best window.  One call warms up, one sizes the window to about 50 ms."""
    fn()
    t1 = window(fn, 1)
    inner = max(1, min(INNER, int(50.0 / max(t1, 1e-3))))
    return min([t1] + [window(fn, inner) for _ in range(repeats)])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    quick = "--quick" in sys.argv
    for K, T, sz in ((100, 4000, (512, 512, 1)), (200, 1000, (512, 512, 2))):
        if quick:
            K, T, sz = 12, 200, (64, 64, 1)
        rng = np.random.RandomState(0)
        X, Y, Z = sz
        P = X * Y * Z
        pos = np.stack([rng.uniform(8, X - 8, K), rng.uniform(8, Y - 8, K), np.full(K, 0.5 * (Z - 1))], 1)
        dn = dNMF.DeformableNMF(torch.tensor(sz), K, T, positions=torch.from_numpy(pos).float())
        dn.verbose = False
        if quick:
            dn.spatial_kernel = 'lists'     # twelve 61-voxel boxes in 64 x 64: 'auto' would take the dense form
        dn.C =torch.from_numpy(rng.gamma(2.0, 1.0, (K, T)).astype(np.float32)).cuda()
        A0 = dn.fp.A.clone()
        frames = torch.rand(T, P, device="cuda")
        sl, ly = dn._spatial_lists(), dn.fp.packed_lists(floor=0.0)
        if sl is None:
            raise SystemExit("the list form does not apply to these footprints")
        total = sl["total"]
        A1c, Cs, ws = ops.spatial_accum_lists(frames, dn.C, sl, sz, K)
        t_k5 = best(lambda: ops.spatial_accum_lists(frames, dn.C, sl, sz, K, A1c=A1c, Cs=Cs, workspace=ws), repeats)
        A = A0.reshape(P, K).clone()
        ent = torch.empty_like(A1c)

        def mu():
            ent.copy_(A1c)
            ops.mu_spatial_lists(A, ly, sl, ent, Cs, sz)

        def hals(sweeps):
            ent.copy_(A1c)
            ops.hals_spatial_lists(A, ly, sl, ent, Cs, sz, sweeps=sweeps)

        t_copy = best(lambda: ent.copy_(A1c), repeats)
        t_mu = best(mu, repeats)
        t_h = {s: best(lambda s=s: hals(s), repeats) for s in (1, 5, 20)}

        def steps_mu():
            dn.fp.A = A0.clone()
            dn._footprints_written()
            for _ in range(5):
                dn.spatial_step(frames)

        def step_hals():
            dn.fp.A = A0.clone()
            dn._footprints_written()
            dn.spatial_step(frames, solver='hals', sweeps=5)

        t_steps_mu = min(window(steps_mu, 1) for _ in range(repeats + 1))
        t_step_hals = min(window(step_hals, 1) for _ in range(repeats + 1))
        kkt = dn.last_spatial_kkt
        floor = 3 * 4.0 * total / HBM_ROOF * 1e3
        print(f"K={K} T={T} {X}x{Y}x{Z}: total {total} entries ({total / P:.2f} per voxel); list K5 {t_k5:.3f} ms; copy of the sums "
              f"{t_copy:.4f} ms; mu_spatial_lists {t_mu:.3f} ms; K6h 1 / 5 / 20 sweeps {t_h[1]:.3f} / {t_h[5]:.3f} / {t_h[20]:.3f} ms "
              f"(floor {floor:.4f} ms at 8 TB/s: {floor / t_h[1]:.3f} / {floor / t_h[5]:.3f} / {floor / t_h[20]:.3f} of it); "
              f"5 x spatial_step('mu') {t_steps_mu:.2f} ms; 1 x spatial_step('hals', sweeps=5) {t_step_hals:.2f} ms "
              f"(kkt max {float(kkt.max()):.3e} median {float(kkt.median()):.3e})", flush=True)
        del dn, frames
        if quick:
            break


if __name__ == "__main__":
    main()
