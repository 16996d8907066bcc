#!/usr/bin/env python3
"""Time K19 (the rank-1 background: dnmf_background_dots, dnmf_background_accum, dnmf_background_subtract) with HIP events,
beside the torch composition of the same steps, in the same run:
python tools/time_background.py [repeats] [--quick] [--rank R[,R...]]

512x512x1 with 4000 frames and 512x512x2 with 1000, with and without ``sub``.  Prints per case the best time of each kernel and
its share of the HBM floor at the 8 TB/s roof: the half-steps read 4 bytes per voxel and frame (8 with ``sub``), the subtraction
reads 4 and writes 4.  The torch composition is what a user without the kernels would chain, in fp32: materialise the residual
``Y - M`` (with ``sub`` only), one ``mv`` per half-step with the clamp and the division, and ``addcmul`` + ``clamp_`` for the
subtraction.  ``--quick``: 64 frames (a rehearsal of the script, not a measurement).

``--rank R`` (2 .. 8, several with commas): also one alternation of the rank-R background of K23 (``dnmf_background_dots_rank`` +
``dnmf_background_accum_rank``, three sweeps) and its subtraction on the same buffers, beside K19's alternation of the same run:
the half-steps still read 4 (8) bytes per voxel and frame, whatever R is."""
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


def torch_iteration(frames, sub, b):
    """One (f-step, b-step) pair in fp32 -> (b, f)."""
    r = frames - sub if sub is not None else frames
    f = torch.mv(r, b).clamp_(min=0).div_(torch.dot(b, b))
    return torch.mv(r.t(), f).clamp_(min=0).div_(torch.dot(f, f)), f


def torch_subtract(frames, b, f, out):
    return torch.addcmul(frames, f[:, None], b[None, :], value=-1.0, out=out).clamp_(min=0)


def time_rank(R, name, frames, sub, sz, out, repeats, k19):
    """One alternation and the subtraction of the rank-R background; ``k19``: {with_sub: K19's alternation in ms}."""
    T, P = frames.shape
    torch.manual_seed(R)
    b = 0.5 + torch.rand(R, P, device="cuda")
    f = 0.5 + torch.rand(R, T, device="cuda")
    state = ops.background_state_rank(sz, T, R)
    for with_sub in (False, True):
        m = sub if with_sub else None
        floor_ms = (8.0 if with_sub else 4.0) * P * T / HBM_ROOF * 1e3
        td = best(lambda: ops.background_dots_rank(frames, b, f, sub=m), repeats)
        ta = best(lambda: ops.background_accum_rank(frames, f, sz, b=b, sub=m, state=state), repeats)
        tag = ", sub" if with_sub else ""
        print(f"{name}{tag}, rank {R}: dots {td:.3f} ms ({floor_ms / td:.2f} of the HBM floor of {floor_ms:.3f} ms), accum {ta:.3f} ms "
              f"({floor_ms / ta:.2f}), one alternation {td + ta:.3f} ms = {(td + ta) / k19[with_sub]:.2f} x K19's {k19[with_sub]:.3f} ms",
              flush=True)
    floor_ms = 8.0 * P * T / HBM_ROOF * 1e3
    ts = best(lambda: ops.background_subtract_rank(frames, b, f, out=out), repeats)
    print(f"{name}, rank {R}: subtract {ts:.3f} ms ({floor_ms / ts:.2f} of the HBM floor of {floor_ms:.3f} ms)", flush=True)


def main():
    argv = sys.argv[1:]
    ranks = []
    if "--rank" in argv:
        at = argv.index("--rank")
        ranks = [int(r) for r in argv[at + 1].split(",")]
        del argv[at:at + 2]
    args = [a for a in argv if not a.startswith("--")]
    repeats = int(args[0]) if args else 5
    quick = "--quick" in argv
    for sz, T in (([512, 512, 1], 4000), ([512, 512, 2], 1000)):
        if quick:
            T = 64
        P = sz[0] * sz[1] * sz[2]
        name = f"{sz[0]}x{sz[1]}x{sz[2]} x {T} frames"
        torch.manual_seed(0)
        frames = 1.0 + torch.rand(T, P, device="cuda")
        sub = torch.rand(T, P, device="cuda")
        b = 0.5 + torch.rand(P, device="cuda")
        f = 0.5 + torch.rand(T, device="cuda")
        out = torch.empty_like(frames)
        state = ops.background_state(sz, T)
        k19 = {}
        for with_sub in (False, True):
            m = sub if with_sub else None
            floor_ms = (8.0 if with_sub else 4.0) * P * T / HBM_ROOF * 1e3
            td = best(lambda: ops.background_dots(frames, b, sub=m), repeats)
            ta = best(lambda: ops.background_accum(frames, f, sz, sub=m, state=state), repeats)
            tt = best(lambda: torch_iteration(frames, m, b), min(repeats, 3))
            k19[with_sub] = td + ta
            tag = ", sub" if with_sub else ""
            print(f"{name}{tag}: dots {td:.3f} ms ({floor_ms / td:.2f} of the HBM floor of {floor_ms:.3f} ms), accum {ta:.3f} ms "
                  f"({floor_ms / ta:.2f}), one iteration {td + ta:.3f} ms; torch composition (fp32) {tt:.3f} ms", flush=True)
            fk = ops.background_dots(frames, b, sub=m)[0]
            bk = ops.background_accum(frames, fk, sz, sub=m, state=state)[0][0].reshape(-1)
            bt, ft = torch_iteration(frames, m, b)
            print(f"{name}{tag}: largest relative difference between the composition and K19: f {float(((ft - fk) / fk).abs().max()):.2e}, "
                  f"b {float(((bt - bk) / bk).abs().max()):.2e}", flush=True)
            del bt, ft
        floor_ms = 8.0 * P * T / HBM_ROOF * 1e3
        ts = best(lambda: ops.background_subtract(frames, b, f, out=out), repeats)
        tt = best(lambda: torch_subtract(frames, b, f, out), min(repeats, 3))
        print(f"{name}: subtract {ts:.3f} ms ({floor_ms / ts:.2f} of the HBM floor of {floor_ms:.3f} ms); torch addcmul + clamp_ "
              f"{tt:.3f} ms", flush=True)
        for R in ranks:
            time_rank(R, name, frames, sub, sz, out, repeats, k19)
        del frames, sub, out, state


if __name__ == "__main__":
    main()
