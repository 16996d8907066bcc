#!/usr/bin/env python3
"""The position initialiser end to end: simulate a moving video, register it piecewise-rigidly (``MotionCorrect``, the
class of the reference's ``Demix/MotionCorrect.py``, on the GPU), move the first frame's neuron centres by the shifts of
their patches (``apply_shifts_points``) and compare with the simulator's own per-frame centres; then start the warp of a
``DeformableNMF`` from those tracks (``init_motion``), fit, and read the tracks (``positions``) and the traces back.  Needs an
MI355X.

    python examples/init_positions.py [--size 128] [--neurons 30] [--frames 50] [--stride 12] [--detect] [--track [--exclude R]] [--follow]
                                      [--gn [--motion-smooth S] [--motion-order ORDER] [--motion-jacobian W]]
                                      [--detect-image {template,corr,max,std,temporal_median,pnr,corr_pnr}]

``--detect``: the centres come from the registration template (``MotionCorrect.detect_points``, K14) instead of the simulator's
ground truth of frame 0; the model is built on the detected centres alone, as many neurons as were found.  The simulator's
centres then serve only to judge the result: a detected centre is matched to the simulated neuron nearest to it in frame 0
when that is within sigma (one centre per neuron), and the errors and correlations are taken over the matched ones.

``--detect-image corr | max | std`` (implies ``--detect``): the centres come from that summary image of the corrected movie
(``MotionCorrect.summary_images``, K18; the registration then keeps its movie, ``save_corrected=True``) instead of the template,
which averages over time.  ``temporal_median | pnr | corr_pnr`` take the temporal median, the peak-to-noise image
(``MotionCorrect.robust_images``, K30) or K18's ``corr`` times it, the usual seed image.  The same three numbers are printed for
the chosen image; with the three K30 images they are unmeasured (the example has not been run with them).

``--track``: the initialiser's tracks are refined per neuron and frame by the tracker (``MotionCorrect.track_points``, K15: the
peak of the matched-filter score within 3 voxels of the patch grid's track) before ``init_motion``; the same three numbers are
printed for both sets of tracks.  ``--exclude R`` (with ``--track``): the tracker takes the neurons already placed in a frame off
the data before it looks for the next one, in R rounds (K15x, ``track_positions(..., exclude=R)``), so a neuron next to a
brighter one is not captured by it; the numbers with it are unmeasured.

``--follow``: the centres of frame 0 are followed through the video by the chained tracker (``ExponentialFP.follow_positions``,
K15c: every frame searched within ``--search`` voxels of what the frame before gave, no registration involved) and the same
three numbers are printed with ``init_motion`` fed from those tracks; the numbers with it are unmeasured.

``--gn``: every fit is repeated with the Gauss-Newton motion solver (``fit(..., motion_solver='gn')``: K16 + Levenberg-Marquardt
steps per frame, ``--gn-iters`` of them, no learning rate) and its three numbers are printed beside Adam's.  ``--motion-smooth S``
gives that fit the temporal prior (``fit(..., motion_smooth=S)``, K16s: S in mean squared error per squared voxel of
frame-to-frame change of a warp coefficient); the numbers with it are unmeasured.  ``--motion-order ORDER`` fits only the
coefficients of that order -- ``translation``, ``affine``, ``quadratic`` (the default: all) -- or, with ``graded``, the three in
turn with ``--gn-iters`` iterations each (``fit(..., motion_order=ORDER)``, K16o); the numbers with it are unmeasured too.
``--motion-jacobian W`` gives that fit the volume-preserving prior (``fit(..., motion_jacobian=W)``, K16j: W in mean squared error
per squared unit of log det J at the corners and the centre of the volume; a step to a map that folds there is never accepted) and
prints the smallest det J the fit ends with; the numbers with it are unmeasured as well.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from Demix.dNMF import DeformableNMF, ExponentialFP, SimulatedVideoDataset  # noqa: E402
from Demix.MotionCorrect import MotionCorrect  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--neurons", type=int, default=30)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--stride", type=int, default=12, help="patch stride in x and y (patches of 1.5 strides; default 12: the simulator's motion varies over ~10 voxels)")
    ap.add_argument("--ridge", type=float, default=1e-3, help="pull of init_motion's fit to the identity")
    ap.add_argument("--lr", type=float, default=1e-6, help="Adam step of the motion update")
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--detect", action="store_true", help="find the centres in the template instead of taking the simulator's")
    ap.add_argument("--detect-image", choices=("template", "corr", "max", "std", "temporal_median", "pnr", "corr_pnr"), default=None,
                    help="--detect on this image: the registration template, a summary image (K18) or an order-statistic image (K30) "
                         "of the corrected movie")
    ap.add_argument("--track", action="store_true", help="refine the initialiser's tracks with the tracker (K15) before init_motion")
    ap.add_argument("--exclude", type=int, default=0, help="--track: rounds of exclusive tracking (K15x); 0: K15 as it is")
    ap.add_argument("--follow", action="store_true", help="follow the centres of frame 0 frame to frame (K15c) and start a fit from those tracks")
    ap.add_argument("--momentum", type=float, default=0.0, help="--follow: share of the last step the next search is moved by")
    ap.add_argument("--gn", action="store_true", help="repeat every fit with the Gauss-Newton motion solver")
    ap.add_argument("--gn-iters", type=int, default=10, help="--gn: Levenberg-Marquardt iterations per frame")
    ap.add_argument("--motion-smooth", type=float, default=0.0, help="--gn: weight of the temporal smoothness prior (0: none)")
    ap.add_argument("--motion-order", choices=("translation", "affine", "quadratic", "graded"), default="quadratic",
                    help="--gn: the coefficients the fit moves; graded: translation, then affine, then all")
    ap.add_argument("--motion-jacobian", type=float, default=0.0, help="--gn: weight of the volume-preserving prior (0: none)")
    ap.add_argument("--gsig", type=float, default=None, help="register on high-pass-filtered frames: gSig_filt=(S, S) (K22)")
    ap.add_argument("--search", type=int, default=3, help="--track, --follow: voxels searched in x and y around the prediction")
    a = ap.parse_args()
    a.detect = a.detect or a.detect_image is not None
    if a.motion_smooth and not a.gn:
        ap.error("--motion-smooth needs --gn (the Adam fit has no temporal term)")
    if a.motion_jacobian and not a.gn:
        ap.error("--motion-jacobian needs --gn (the Adam fit's reg term carries no gradient)")
    if a.motion_order != "quadratic" and not a.gn:
        ap.error("--motion-order needs --gn (the Adam fit steps on all of beta)")
    image = a.detect_image or "template"
    torch.manual_seed(0)
    np.random.seed(0)
    K, T, sz = a.neurons, a.frames, torch.tensor([a.size, a.size, 2])
    dataset = SimulatedVideoDataset(K=K, T=T, sz=sz, shape_std=3, density=.2, bg_snr=-120, motion='gp', traces='exp',
                                    motion_par={'sigma': [5, 5, .01], 'ls': [10, 10, 10]})
    video = np.moveaxis(np.asarray(dataset.video), -1, 0)            # (X, Y, Z, T) -> (T, X, Y, Z)
    truth = np.asarray(dataset.positions)                            # (K, 3, T)
    stride = a.stride
    mc = MotionCorrect(video, max_shifts=(12, 12, 1), strides=(stride, stride, 1), overlaps=(stride // 2, stride // 2, 1),
                       max_deviation_rigid=3, is3D=True, pw_rigid=True, save_corrected=image != "template",
                       gSig_filt=None if a.gsig is None else (a.gsig, a.gsig))
    mc.motion_correct()                                              # template=None: rigid pass first
    # pts: the centres the tracks start from; sel / tr: rows of pts and the simulated neurons they are judged against
    if a.detect:
        shape_std = 3.0
        pts = mc.detect_points(K, shape_std=shape_std, image=image)  # (n, 3), brightest first
        d = np.linalg.norm(pts[:, None, :2] - truth[None, :, :2, 0], axis=2)     # in the plane, like the errors below
        nearest = d.argmin(1)
        sel = np.array([j for j in range(len(pts)) if d[j, nearest[j]] <= shape_std and j == d[:, nearest[j]].argmin()], dtype=int)
        tr = nearest[sel]
        if len(sel) == 0:
            raise SystemExit(f"detect_points (image={image!r}): {len(pts)} centres, none within {shape_std:g} voxels of a simulated neuron")
        print(f"detect_points (image={image!r}): {len(pts)} centres; {len(sel)} of the simulator's {K} neurons have one within "
              f"{shape_std:g} voxels, mean distance of those {d[sel, tr].mean():.2f} voxels")
    else:
        pts, sel, tr = truth[:, :, 0], np.arange(K), np.arange(K)
    n = len(pts)
    P_T = mc.apply_shifts_points(video, pts)                         # (n, 3, T)
    still = np.abs(truth[tr, :2, :] - truth[tr, :2, :1]).mean()      # error of "the neurons do not move"
    err = np.abs(P_T[sel, :2, :] - truth[tr, :2, :]).mean()
    print(f"video {tuple(video.shape)}, {len(mc.x_shifts_els[0])} patches; rigid shifts up to "
          f"{np.abs(np.array(mc.shifts_rig)).max():.1f} voxels")
    print(f"mean |x, y error| of the per-frame centres: {err:.2f} voxels with the initialiser, {still:.2f} without")
    # the tracks enter the model (init_motion), and come out of it again (positions): one fit from the identity warp and
    # one from the warp the tracks imply, each judged by where it puts the neurons and by its traces
    from dnmf_amd.WUtils.Simulator import get_roi_signals

    def median_corr(S):
        return float(np.median([np.corrcoef(S[j], dataset.traces[k])[0, 1] for j, k in zip(sel, tr)]))

    starts = {"identity": None, "tracks": P_T}
    if a.track:
        refined, _ = mc.track_points(video, pts, search=(a.search, a.search, 1), shape_std=3, exclude=a.exclude)
        lost = np.isnan(refined).any(1)
        print(f"track_points: {int((~lost).sum())} of {lost.size} (neuron, frame) pairs found; mean |x, y error| of the per-frame "
              f"centres {np.nanmean(np.abs(refined[sel, :2, :] - truth[tr, :2, :])):.2f} voxels with the tracker, {err:.2f} with "
              f"the initialiser alone")
        starts["tracker"] = refined
    if a.follow:
        chained, _, info = ExponentialFP.follow_positions(video, pts, shape_std=3, search=(a.search, a.search, 1), anchor=0,
                                                          momentum=a.momentum)
        lost = np.isnan(chained).any(1)
        print(f"follow_positions: {int((~lost).sum())} of {lost.size} (neuron, frame) pairs found, {int((info['lost_at'] >= 0).sum())} "
              f"chains lost; mean |x, y error| of the per-frame centres {np.nanmean(np.abs(chained[sel, :2, :] - truth[tr, :2, :])):.2f} "
              f"voxels chained, {err:.2f} with the initialiser alone")
        starts["chained"] = chained
    for start, tracks in starts.items():
        for solver in ("adam", "gn") if a.gn else ("adam",):
            torch.manual_seed(1)
            dn = DeformableNMF(sz, n, T, positions=torch.from_numpy(P_T[:, :, 0]).float())
            dn.verbose = False
            if tracks is not None:
                ok = dn.init_motion(tracks, ridge=a.ridge)
                print(f"init_motion: {int(ok.sum())} of {T} frames fitted")
            loader = dataset.loader(a.batch)
            if solver == "gn":
                dn.fit(loader, loader, None, a.batch, outer=1, epochs=a.gn_iters, gamma_c=0, iter_c=30, motion_solver='gn',
                       motion_smooth=a.motion_smooth, motion_order=a.motion_order, motion_jacobian=a.motion_jacobian)
                if a.motion_jacobian:
                    print(f"smallest det J at the sample points: {float(dn.last_motion_gn['min_det'].min()):.3f}")
            else:
                dn.fit(loader, loader, torch.optim.Adam([dn.fp.beta], lr=a.lr), a.batch, outer=1, epochs=a.epochs, gamma_c=0, iter_c=30)
            where = dn.positions()
            dist = float(np.nanmean(np.linalg.norm(where[sel, :2, :] - truth[tr, :2, :], axis=1)))
            # the simulator places centres up to half a voxel beyond the last slice: read the box of the nearest voxel inside
            inside = np.clip(np.nan_to_num(where, nan=-1.0), 0, (sz.numpy() - 1)[None, :, None])
            roi = get_roi_signals(dataset.video, torch.from_numpy(inside), np.array([3, 3, 0]))
            label = start
            if solver == "gn":
                label += (f" (gn, {a.gn_iters} iterations" + (f", smooth {a.motion_smooth:g}" if a.motion_smooth else "")
                          + (f", jacobian {a.motion_jacobian:g}" if a.motion_jacobian else "")
                          + (f", order {a.motion_order})" if a.motion_order != "quadratic" else ")"))
            print(f"{label} start: mean distance of dnmf.positions() from the simulator's centres {dist:.2f} voxels; median "
                  f"correlation with the simulator's traces: dnmf.C {median_corr(dn.C.cpu().numpy()):.3f}, ROI traces on "
                  f"dnmf.positions() {median_corr(np.nan_to_num(roi)):.3f}")
    return err, still


if __name__ == "__main__":
    main()
