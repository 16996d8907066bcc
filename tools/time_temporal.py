#!/usr/bin/env python3
"""Time the two trace solvers on the slot tables of K3n: K4 (multiplicative update, ops.mu_temporal_slots) at
iter_c = 50, and K4h (exact coordinate descent, ops.hals_temporal_slots) at the number of sweeps after which its
objective F = sum_t 1/2 c^T G c - r^T c is at or below K4's:
python tools/time_temporal.py [repeats] [T]

Cases: the bench video (512x512x1, K = 100, T = 4000 simulated frames) and a 512x512x2 volume, each after one motion
epoch from the identity (so the warp is the one a fit would read the traces under).  The Gram data are made once (K3n,
finish=False for the slot tables, finish=True for the dense G, r on which F and the convergence measure are evaluated
in float64); both solvers start from the same traces.  Prints ms per call (HIP events around the call, best of
`repeats`, wrapper included), F, the max / median of the per-frame convergence measure (kkt) and the number of
non-finite traces of both; nothing is asserted about time.  Where K4 leaves non-finite or unbounded traces (see objective())
its F is not a target K4h can or should meet, and the search reports that after 50 sweeps.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402
from dnmf_amd.Demix import dNMF as M  # noqa: E402
from dnmf_amd.WUtils import Simulator  # noqa: E402


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def objective(G, r, C, step=500):
    """F in float64 on the device, `step` frames at a time.  Non-finite traces count as 0 (report() prints how many there
    are: the multiplicative update divides by G c + 1e-32, and a neuron whose footprint has all but left the volume can
    have G[k,k] underflow to 0 while r[k] has not -- its trace then grows by 1e7 a round)."""
    C = torch.nan_to_num(C, nan=0.0, posinf=0.0, neginf=0.0)
    f = 0.0
    for s in range(0, r.shape[0], step):
        g, c = G[s:s + step].double(), C[:, s:s + step].double().T.contiguous()      # (t,K,K), (t,K)
        f += float((0.5 * torch.einsum("tk,tkl,tl->", c, g, c) - (r[s:s + step].double() * c).sum()))
    return f


def kkt_of(G, r, C, nbr):
    C = torch.nan_to_num(C, nan=0.0, posinf=0.0, neginf=0.0)
    return ops.hals_temporal_kkt(G, r, C.double().contiguous(), 0.0, nbr=nbr)


def case(name, sz, K, T, repeats):
    torch.manual_seed(0)
    np.random.seed(0)
    frames, positions, _ = Simulator.generate_video_resident(K, T, sz, 3, .2, -120, {"sigma": [5, 5, .01], "ls": [10, 10, 10]})
    frames.clamp_(min=0)
    dn = M.DeformableNMF(torch.tensor(sz), K, T, positions=positions[:, :, 0].contiguous())
    dn.verbose = False
    opt = torch.optim.Adam([dn.fp.beta], lr=1e-5)
    train = M.ResidentLoader(frames, sz, 4, shuffle=True, generator=torch.Generator().manual_seed(1))
    dn.update_motion(train, opt, gamma=1, epochs=1)
    fp = dn.fp
    ly = dn._lists_layout_for_fused_update(0)
    if ly is None:
        print(f"{name}: the slot path does not apply to these footprints")
        return
    fr, order = dn._gather_frames(M.ResidentLoader(frames, sz, 4))
    beta = fp.beta.detach()
    G, r, _ = ops.warp_gram_rhs_lists(ly, K, fp.sz_list, beta, order, fr)
    _, _, ws = ops.warp_gram_rhs_lists(ly, K, fp.sz_list, beta, order, fr, finish=False)
    C0 = dn.C.to("cuda", torch.float32)[:, order.long()].contiguous()
    nbr = ly["nbr"]
    print(f"{name}: K = {K}, T = {T}, {sz[0]}x{sz[1]}x{sz[2]}, NN = {nbr.shape[1]}, F(start) = {objective(G, r, C0):.9g}")

    def report(label, C, ms):
        k = kkt_of(G, r, C, nbr)
        print(f"  {label}: {ms:.3f} ms per call, F = {objective(G, r, C):.12g}, kkt max {float(k.max()):.3e} "
              f"median {float(k.median()):.3e}, non-finite traces {int((~torch.isfinite(C)).sum())}", flush=True)

    Cmu = ops.mu_temporal_slots(ly, ws, fp.sz_list, C0.clone(), 50)
    f_mu = objective(G, r, Cmu)
    report("K4  mu_temporal_slots, 50 rounds", Cmu, timed(lambda: ops.mu_temporal_slots(ly, ws, fp.sz_list, C0.clone(), 50), repeats))
    print("  (a clone of C is inside both timings: %.3f ms)" % timed(lambda: C0.clone(), repeats))
    match = None
    for sweeps in range(1, 51):
        if objective(G, r, ops.hals_temporal_slots(ly, ws, fp.sz_list, C0.clone(), sweeps)) <= f_mu:
            match = sweeps
            break
    if match is None:
        print("  K4h is still above K4's F after 50 sweeps")
        match = 50
    for sweeps in sorted({match, 10, 50}):
        Ch = ops.hals_temporal_slots(ly, ws, fp.sz_list, C0.clone(), sweeps)
        tag = " (first at or below K4's F)" if sweeps == match else ""
        report(f"K4h hals_temporal_slots, {sweeps} sweeps{tag}", Ch,
               timed(lambda: ops.hals_temporal_slots(ly, ws, fp.sz_list, C0.clone(), sweeps), repeats))
    report(f"K4h hals_temporal (dense G + nbr), {match} sweeps", ops.hals_temporal(G, r, C0.clone(), match, nbr=nbr),
           timed(lambda: ops.hals_temporal(G, r, C0.clone(), match, nbr=nbr), repeats))
    report(f"K4h hals_temporal (dense G), {match} sweeps", ops.hals_temporal(G, r, C0.clone(), match),
           timed(lambda: ops.hals_temporal(G, r, C0.clone(), match), repeats))
    report("K4  mu_temporal (dense G + nbr), 50 rounds", ops.mu_temporal(G, r, C0.clone(), 50, nbr=nbr),
           timed(lambda: ops.mu_temporal(G, r, C0.clone(), 50, nbr=nbr), repeats))


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 4000
    case("bench video", [512, 512, 1], 100, T, repeats)
    case("two slices", [512, 512, 2], 100, T, repeats)


if __name__ == "__main__":
    main()
