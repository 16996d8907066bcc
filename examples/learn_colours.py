#!/usr/bin/env python3
"""Colour learning end to end (K29): simulate a moving video, render it in three channels with planted colours -- channel c shows
neuron k with ``colours[c, k]`` times its light, the renderer of the simulator's resident video run once per channel on the
simulator's own positions and traces -- build a ``MultiChannelDNMF`` that knows nothing about the colours (all ones), run
``fit(..., learn_colours=10)`` and print the largest colour error before and after.  Needs an MI355X.

    python examples/learn_colours.py [--size 64] [--neurons 12] [--frames 40] [--outer 3]

The planted colours are drawn in [0.1, 1] and scaled so that every neuron's largest colour is 1, the normal form
``update_colours`` leaves; a colour and its trace share one scale, so only that form can be compared.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dnmf_amd import ops  # noqa: E402
from dnmf_amd.Demix.dNMF import MultiChannelDNMF, ResidentLoader, SimulatedVideoDataset  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--neurons", type=int, default=12)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--outer", type=int, default=3)
    ap.add_argument("--lr", type=float, default=1e-6, help="Adam step of the motion update")
    ap.add_argument("--batch", type=int, default=10)
    a = ap.parse_args()
    torch.manual_seed(0)
    np.random.seed(0)
    NC, K, T = 3, a.neurons, a.frames
    sz = torch.tensor([a.size, a.size, 2])
    szl = [a.size, a.size, 2]
    dataset = SimulatedVideoDataset(K=K, T=T, sz=sz, shape_std=3, density=.2, bg_snr=-120, motion='gp', traces='exp',
                                    motion_par={'sigma': [5, 5, .01], 'ls': [10, 10, 10]})
    positions = torch.as_tensor(np.asarray(dataset.positions)).to("cuda", torch.float32).contiguous()     # (K, 3, T)
    traces = torch.as_tensor(np.asarray(dataset.traces)).to("cuda", torch.float64).contiguous()           # (K, T)
    rng = np.random.default_rng(0)
    colours = rng.uniform(0.1, 1.0, (NC, K))
    colours /= colours.max(axis=0, keepdims=True)
    planted = torch.from_numpy(colours).cuda()
    frames = torch.cat([ops.render_frames(positions, (traces * planted[c][:, None]).contiguous(), szl, 3.0) for c in range(NC)], 1)
    dn = MultiChannelDNMF(sz, K, T, torch.ones(NC, K), positions=positions[:, :, 0].cpu())
    dn.verbose = False
    before = float((dn.colours.double() - planted).abs().max())
    train = ResidentLoader(frames, szl, a.batch, shuffle=True, generator=torch.Generator().manual_seed(0))
    test = ResidentLoader(frames, szl, a.batch)
    dn.fit(train, test, torch.optim.Adam([dn.fp.beta], lr=a.lr), a.batch, outer=a.outer, epochs=2, gamma_c=0, iter_c=30,
           learn_colours=10)
    after = float((dn.colours.double() - planted).abs().max())
    last = dn.last_colours
    print(f"video {tuple(frames.shape)} = {T} frames of {NC} channels x {a.size}x{a.size}x2, {K} neurons")
    print(f"largest colour error: {before:.3f} with all-ones colours, {after:.3f} after fit(learn_colours=10); kkt of the last "
          f"update {float(last['kkt'].max()):.2e}, neurons updated {int(last['ok'].sum())} of {K}")
    return before, after


if __name__ == "__main__":
    main()
