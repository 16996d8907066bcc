#!/usr/bin/env python3
"""Times of the Gauss-Newton motion solver beside the Adam path, 512x512x1 and 512x512x2, K = 100, T = 4000, warp about a voxel
off the identity (bench.py's ``displaced_beta``):

  kernels    K16 (``ops.warp_normal_eqs``) alone beside K2 (``ops.warp_recon_grad``) alone on the same frames and images:
             both read exactly the same bytes, so the ratio is the cost of K16's extra sums
  iteration  one Levenberg-Marquardt iteration (K16 + ``ops.lm_step``; from ``update_motion(solver='gn')`` with 5 and with 1
             iterations) beside one Adam epoch of ``update_motion`` (reconstruction + K2 + ``adam_epoch``)

  --smooth S an LM iteration with the temporal prior (``model.motion_smooth = S``, ``update_motion(solver='gn')``: the same
             work in twice the launches, ``dnmf_lm_step_smooth``) beside the one without, in the ``iteration`` line
  --order O  ``steps``: the step alone on K16's output -- ``dnmf_lm_step`` beside ``dnmf_lm_step_order`` at ``translation``,
             ``affine`` and ``quadratic`` (3 / 12 / 30 unknowns; 2 / 6 / 12 at Z = 1) -- and, for O other than ``quadratic``, an LM
             iteration with ``model.motion_order = O`` in the ``iteration`` line (``graded``: a round of its three stages)

  --jacobian W  ``steps``: the step with the volume-preserving prior (``ops.lm_step(jacobian=W)``, ``dnmf_lm_step_jac``) beside
             the plain ``dnmf_lm_step`` on the same K16 output, and an LM iteration with ``model.motion_jacobian = W`` in the
             ``iteration`` line

    python tools/time_motion_gn.py [--frames 4000] [--neurons 100] [--smooth 1e-4] [--order graded] [--jacobian 1e-3]

Every measurement is a process of its own under a time limit; the first one that fails ends the script.  One JSON line each.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, warm=2, reps=5):
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def setup(Z, K, T):
    import torch
    from bench import displaced_beta
    from dnmf_amd.Demix import dNMF
    torch.manual_seed(0)
    sz = [512, 512, Z]
    pos = torch.rand(K, 3) * torch.tensor([511.0, 511.0, float(Z - 1)])
    model = dNMF.DeformableNMF(torch.tensor(sz), K, T, positions=pos)
    model.verbose = False
    with torch.no_grad():
        model.fp.beta.copy_(displaced_beta(T, sz, "cuda"))
    frames = torch.rand((T, 512 * 512 * Z), device="cuda")
    return dNMF, model, sz, frames


def step_kernels(Z, K, T):
    import torch
    from dnmf_amd import ops
    _, model, sz, frames = setup(Z, K, T)
    S = model._recon_cache()[0]
    times = torch.arange(T, dtype=torch.int32, device="cuda")
    beta = model.fp.beta.detach()
    grad = torch.zeros_like(beta)
    ws = {}

    def k2():
        ws["k2"] = ops.warp_recon_grad(S, times, frames, None, sz, beta, times, grad=grad, want_loss=False, want_reg=False,
                                       workspace=ws.get("k2"))["workspace"]

    def k16():
        ws["eq"] = ops.warp_normal_eqs(S, times, frames, None, sz, beta, times, out=ws.get("eq"), workspace=ws.get("k16"))
        ws["k16"] = ws["eq"]["workspace"]

    t2, t16 = median_ms(k2), median_ms(k16)
    return {"step": "kernels", "Z": Z, "K": K, "T": T, "k2_ms": t2, "k16_ms": t16, "ratio": t16 / t2}


def step_steps(Z, K, T, jacobian=0.0):
    """The step alone, B = T frames: one K16 evaluation, then each entry on a fresh state (the first call: accept + solve)."""
    import torch
    from dnmf_amd import _lib, ops
    _, model, sz, frames = setup(Z, K, T)
    S = model._recon_cache()[0]
    times = torch.arange(T, dtype=torch.int32, device="cuda")
    beta = model.fp.beta.detach()
    start = beta.clone()
    eqs = ops.warp_normal_eqs(S, times, frames, None, sz, beta, times)
    state = ops.lm_state(T, "cuda")
    M, Minv = ops._centred(sz, beta.device)
    lib = _lib.load()

    def run(order):
        state["counts"].zero_()
        beta.copy_(start)
        if order is None:
            ops.lm_step(state, eqs, sz, beta, times)
            return
        rc = lib.dnmf_lm_step_order(eqs["H"].data_ptr(), eqs["g"].data_ptr(), eqs["sse"].data_ptr(), T, Z, order, M.data_ptr(),
                                    Minv.data_ptr(), beta.data_ptr(), T, times.data_ptr(), state["H"].data_ptr(),
                                    state["g"].data_ptr(), state["sse"].data_ptr(), state["sse0"].data_ptr(), state["lam"].data_ptr(),
                                    state["beta"].data_ptr(), state["counts"].data_ptr(), 10.0, 1e-3, 1e-9, 1e9, 0, None, 0.0, None,
                                    ops._stream())
        _lib.check(rc, "dnmf_lm_step_order")

    out = {"step": "steps", "Z": Z, "K": K, "T": T, "lm_step_ms": median_ms(lambda: run(None))}
    for name, order in ops.WARP_ORDERS.items():
        out[f"lm_step_order_{name}_ms"] = median_ms(lambda: run(order))
    if jacobian:
        def run_jac():
            state["counts"].zero_()
            beta.copy_(start)
            ops.lm_step(state, eqs, sz, beta, times, jacobian=jacobian)

        out.update(jacobian=jacobian, lm_step_jac_ms=median_ms(run_jac))
    return out


def step_iteration(Z, K, T, smooth=0.0, order="quadratic", jacobian=0.0):
    import torch
    dNMF, model, sz, frames = setup(Z, K, T)
    loader = dNMF.ResidentLoader(frames, sz, 100)
    start = model.fp.beta.detach().clone()
    opt = torch.optim.Adam([model.fp.beta], lr=1e-5 * (50 / 512) ** 2)

    def reset():
        with torch.no_grad():
            model.fp.beta.copy_(start)

    def wall(fn, reps=3):
        ts = []
        for _ in range(reps + 1):
            reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts[1:])[len(ts[1:]) // 2]     # the first run warms up

    adam = wall(lambda: model.update_motion(loader, opt, epochs=1))
    gn1 = wall(lambda: model.update_motion(loader, None, solver='gn', iters=1))
    gn5 = wall(lambda: model.update_motion(loader, None, solver='gn', iters=5))
    out = {"step": "iteration", "Z": Z, "K": K, "T": T, "adam_epoch_ms": adam, "gn_iters1_ms": gn1, "gn_iters5_ms": gn5,
           "lm_iteration_ms": (gn5 - gn1) / 4}
    if smooth:
        model.motion_smooth = smooth
        s1 = wall(lambda: model.update_motion(loader, None, solver='gn', iters=1))
        s5 = wall(lambda: model.update_motion(loader, None, solver='gn', iters=5))
        model.motion_smooth = 0.0
        out.update(smooth=smooth, gn_smooth_iters1_ms=s1, gn_smooth_iters5_ms=s5, lm_smooth_iteration_ms=(s5 - s1) / 4)
    if order != "quadratic":
        model.motion_order = order
        o1 = wall(lambda: model.update_motion(loader, None, solver='gn', iters=1))
        o5 = wall(lambda: model.update_motion(loader, None, solver='gn', iters=5))
        model.motion_order = "quadratic"
        out.update(order=order, gn_order_iters1_ms=o1, gn_order_iters5_ms=o5, lm_order_iteration_ms=(o5 - o1) / 4)
    if jacobian:
        model.motion_jacobian = jacobian
        j1 = wall(lambda: model.update_motion(loader, None, solver='gn', iters=1))
        j5 = wall(lambda: model.update_motion(loader, None, solver='gn', iters=5))
        model.motion_jacobian = 0.0
        out.update(jacobian=jacobian, gn_jac_iters1_ms=j1, gn_jac_iters5_ms=j5, lm_jac_iteration_ms=(j5 - j1) / 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--neurons", type=int, default=100)
    ap.add_argument("--step", choices=["kernels", "iteration", "steps"])
    ap.add_argument("--z", type=int, default=1)
    ap.add_argument("--smooth", type=float, default=0.0, help="also time an LM iteration with this temporal prior weight")
    ap.add_argument("--order", choices=["translation", "affine", "quadratic", "graded"], default=None,
                    help="also time the step per warp order, and an LM iteration with this motion_order")
    ap.add_argument("--jacobian", type=float, default=0.0,
                    help="also time the step and an LM iteration with this volume-preserving prior weight")
    ap.add_argument("--limit", type=int, default=240, help="seconds a measurement may take")
    a = ap.parse_args()
    if a.step:
        out = step_kernels(a.z, a.neurons, a.frames) if a.step == "kernels" else step_steps(a.z, a.neurons, a.frames, a.jacobian) \
            if a.step == "steps" else step_iteration(a.z, a.neurons, a.frames, a.smooth, a.order or "quadratic", a.jacobian)
        print(json.dumps(out), flush=True)
        return 0
    for z in (1, 2):
        for step in ("kernels", "iteration") + (("steps",) if a.order or a.jacobian else ()):
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--step", step, "--z", str(z),
                   "--frames", str(a.frames), "--neurons", str(a.neurons), "--smooth", str(a.smooth), "--jacobian", str(a.jacobian)]
            if a.order:
                cmd += ["--order", a.order]
            rc = subprocess.run(cmd, cwd=ROOT).returncode
            if rc != 0:
                print(f"time_motion_gn: {step} at Z={z} ended with status {rc}; stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
