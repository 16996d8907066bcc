#!/usr/bin/env python3
"""Time the footprint update of MultiChannelDNMF at the config-5 per-GPU shard (512x512x1, NC = 3, K = 200):

  K7   the channel K7 (dnmf_image_iwarp_channels: one search, NC gathers) against NC single-channel launches;
  K5   the channel list-form K5 (dnmf_spatial_accum_lists_channels) against the dense K5 by column groups (per channel);
  step a whole update_footprints(live_spatial=True) (temporal updates, channel K7, spatial_step), and its spatial_step.

    python tools/time_multichannel.py [frames=1000] [repeats=5]

Median of the repeats after one warm-up, HIP events around each region.  One JSON line at the end."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402
from dnmf_amd.Demix import dNMF as M  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    T = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    sz, K, NC = [512, 512, 1], 200, 3
    P = 512 * 512
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    pos = torch.from_numpy(rng.rand(K, 3) * np.array([512.0, 512.0, 0.0])).float()
    colours = torch.from_numpy(0.3 + rng.rand(NC, K)).float()
    dn = M.MultiChannelDNMF(torch.tensor(sz), K, T, colours, positions=pos)
    dn.verbose = False
    A = dn.fp.A.reshape(P, K)
    Ctrue = 0.5 + torch.rand(K, T, device="cuda")
    frames = torch.cat([((A * dn.colours[c]) @ Ctrue).T for c in range(NC)], 1).contiguous()   # (T, NC*P)
    frames += 0.05 * torch.rand_like(frames)
    dn.C = 0.5 + torch.rand(K, T, device="cuda")
    # the warps of a fit: sub-voxel shifts, linear terms of 1e-3 (tools/time_iwarp.py's amplitude 0)
    beta = torch.cat((torch.zeros(1, 3), torch.eye(3), torch.zeros(6, 3)), 0)[:, :, None].repeat(1, 1, T).cuda()
    scale = torch.tensor([1.0, 1.0 / 512, 1.0 / 512, 0, 1.0 / 512 ** 2, 1.0 / 512 ** 2, 0, 1.0 / 512 ** 2, 0, 0], device="cuda")
    beta += 0.5 * torch.randn_like(beta) * scale[:, None, None]
    beta[:, 2] = torch.tensor([0, 0, 0, 1.0, 0, 0, 0, 0, 0, 0], device="cuda")[:, None]
    with torch.no_grad():
        dn.fp.beta.copy_(beta)
    beta = dn.fp.beta.detach()
    times = torch.arange(T, dtype=torch.int32, device="cuda")
    res = {"geometry": [512, 512, 1], "NC": NC, "K": K, "T": T}

    # K7
    out = torch.empty((T, NC * P), device="cuda")
    res["k7_channels_ms"] = timed(lambda: ops.image_iwarp(frames, None, sz, beta, times, out=out, nchan=NC), reps)

    def k7_each():
        for c in range(NC):
            ops.image_iwarp(frames[:, c * P:(c + 1) * P], None, sz, beta, times, out=out[:, c * P:(c + 1) * P])

    res["k7_per_channel_ms"] = timed(k7_each, reps)
    res["k7_one_channel_ms"] = timed(lambda: ops.image_iwarp(frames[:, :P], None, sz, beta, times, out=out[:, :P]), reps)

    # K5
    C = dn.C.contiguous()
    sl = ops.spatial_lists_setup(dn.fp.packed_lists(floor=0.0), K, sz)
    assert sl["total"] > 0, "the config-5 footprints should have tile lists"
    A1c = torch.empty((sl["total"],), device="cuda")
    Cs = torch.empty((K, K), device="cuda")
    ws = [None]

    def k5_lists():
        ws[0] = ops.spatial_accum_lists_channels(out, C, dn.colours, sl, sz, K, A1c=A1c, Cs=Cs, workspace=ws[0])[2]

    res["k5_lists_channels_ms"] = timed(k5_lists, reps)
    A1 = torch.empty((P, K), device="cuda")
    part = torch.empty((P, K), device="cuda")

    def k5_dense():
        A1.zero_()
        for c in range(NC):
            M.DeformableNMF._spatial_accum_dense(out[:, c * P:(c + 1) * P], C, part, Cs, None, None)
            A1.addcmul_(part, dn.colours[c][None, :])

    res["k5_dense_groups_ms"] = timed(k5_dense, reps)
    res["k5_buffer_MB"] = {"lists": 4 * (sl["total"] + K * K) / 1e6, "dense": 4 * (P * K + K * K) / 1e6}
    del A1, part

    # a whole update_footprints(live_spatial=True), and its spatial_step alone (gamma_a = 0: D does not enter)
    test = M.ResidentLoader(frames, sz, 100)
    A0, C0 = dn.fp.A.clone(), dn.C.clone()

    def sweep():
        dn.fp.A = A0.clone()
        dn.C = C0.clone()
        dn.update_footprints(test, 100, sz, gamma_c=0, gamma_a=0, iter_c=10, live_spatial=True)

    res["update_footprints_live_spatial_ms"] = timed(sweep, reps)
    res["update_footprints_temporal_only_ms"] = timed(
        lambda: (setattr(dn, "C", C0.clone()), dn.update_footprints(test, 100, sz, gamma_c=0, iter_c=10)), reps)

    def step():
        dn.fp.A = A0.clone()
        dn.spatial_step(dn._reg_buf, gamma=0.0, times=times)

    res["spatial_step_ms"] = timed(step, reps)
    res["spatial_step_form"] = "lists" if dn._spatial_lists() is not None else "dense"
    for k, v in res.items():
        print(f"{k}: {v:.3f}" if isinstance(v, float) else f"{k}: {v}", flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
