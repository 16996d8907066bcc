#!/usr/bin/env python3
"""The fit loop of the reference's demo (simulate -> loaders -> alternate motion / footprint steps) without the
plots, against this repository's drop-in ``Demix.dNMF``.  Prints how well the recovered traces match the ground
truth.  Needs an MI355X.

    python examples/demo_headless.py [--outer 5] [--epochs 10] [--iter-c 50] [--clean FPS] [--deconvolve] [--match]
                                        [--evaluate] [--merge] [--spatial-solver hals [--grow G] [--iter-a N]]
                                        [--clean-footprints] [--add N] [--dff W] [--ar1 [SWEEPS] [--ar-penalty L]] [--denoise]

``--ar1``: after the fit, read the traces out twice from the fitted ``C`` on the same Gram data, with SWEEPS (default 10) sweeps of
the exact solver (``update_footprints(solver='hals')``, K4h) and of the AR(1)-constrained update (``solver='ar1'``, K32: the
simulator's decay e^-0.3, penalty ``--ar-penalty``, the baseline taken from the 'hals' traces), and print the median correlation of
the simulator's traces with ``C`` for each.  The fitted ``C`` is put back afterwards.

``--denoise``: after the fit, denoise the registered movie by local low-rank approximation (``DeformableNMF.denoise_movie``, K34,
``registered='linear'``) and print the median number of components kept per patch and the peak of K18's ``corr`` image on the raw
and on the denoised registered movie.

``--clean FPS``: also clean the traces up (``DeformableNMF.clean_traces``, K20) as if the video ran at FPS frames per second and
print the median correlation of the simulator's traces with ``C`` and with the cleaned ``C``.
``--dff W``: also read the traces against their running 8th-percentile baseline over windows of W frames
(``DeformableNMF.detrend_traces``, K31) and print the median correlation of the simulator's traces with ``C`` and with the detrended ``C``.
``--deconvolve``: also deconvolve the traces (``DeformableNMF.deconvolve``, K21), everything estimated, and print the median
correlation of the simulator's traces with ``C`` and with ``b + c``, and the median estimated decay beside the simulator's e^-0.3.
``--match``: also put the traces in the simulator's units (``DeformableNMF.match_traces``, K25) and print the median over neurons
of the RMS difference between the simulator's traces and ``C`` before and after, beside the correlation, which the map leaves alone.
``--clean-footprints``: after the fit, clean the footprints (``DeformableNMF.clean_footprints``, K27: median, energy cut, closing,
largest part) and print each neuron's box, kept voxels and parts.
``--add N``: after the fit, look for up to N neurons the model has no component for in the residual (``DeformableNMF.add_components``,
K28) and print each candidate's explained / energy and K before and after.
``--merge``: last of all, merge the components that sit on one cell (``DeformableNMF.merge_components``, K26) and print the groups
and K before and after.
``--spatial-solver hals``: also update the footprints after every temporal update (``update_footprints(live_spatial=True)``) with
the exact solver K6h: ``--iter-a`` sweeps (default 5) on supports grown by ``--grow`` voxels (default 0), one K5 pass each time;
``--spatial-solver mu``: ``--iter-a`` multiplicative updates (K6) instead.  Prints the per-neuron KKT figure of the last step.
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.optim as optim
from torch.utils.data import DataLoader

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from Demix.dNMF import DeformableNMF, ExponentialFP, SimulatedVideoDataset  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--outer", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--iter-c", type=int, default=50)
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--clean", type=float, default=None, metavar="FPS")
    ap.add_argument("--dff", type=int, default=0, metavar="W")
    ap.add_argument("--deconvolve", action="store_true")
    ap.add_argument("--match", action="store_true")
    ap.add_argument("--evaluate", action="store_true")
    ap.add_argument("--merge", action="store_true")
    ap.add_argument("--add", type=int, default=0, metavar="N")
    ap.add_argument("--clean-footprints", action="store_true")
    ap.add_argument("--spatial-solver", choices=("mu", "hals"), default=None)
    ap.add_argument("--grow", type=int, default=0)
    ap.add_argument("--iter-a", type=int, default=5)
    ap.add_argument("--ar1", type=int, nargs="?", const=10, default=0, metavar="SWEEPS")
    ap.add_argument("--ar-penalty", type=float, default=0.0)
    ap.add_argument("--denoise", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    np.random.seed(0)
    K, T, sz = 10, 100, torch.tensor([50, 50, 2])
    efp = ExponentialFP(sz, K, T, positions=None, shape_std=3)
    A_tC, A_t, grid, reg = efp(np.arange(3), torch.rand(K, T))
    dataset = SimulatedVideoDataset(K=K, T=T, sz=sz, shape_std=3, density=.2, bg_snr=-120, motion='gp', traces='exp',
                                    motion_par={'sigma': [5, 5, .01], 'ls': [10, 10, 10]})
    batch_size = 4
    dataloader = DataLoader(dataset, batch_size=batch_size, shuffle=True, num_workers=0)
    testloader = DataLoader(dataset, batch_size=batch_size, shuffle=False, num_workers=0)
    dnmf = DeformableNMF(sz, K, T, positions=dataset.positions[:, :, 0])
    dnmf.verbose = not a.quiet
    optimizer = optim.Adam([dnmf.fp.beta], lr=1e-5)
    for _ in range(a.outer):
        dnmf.update_motion(dataloader, optimizer, gamma=1, epochs=a.epochs)
        spatial = {} if a.spatial_solver is None else dict(live_spatial=True, spatial_solver=a.spatial_solver, iter_a=a.iter_a,
                                                           grow=a.grow)
        A_t, Y_i, Y = dnmf.update_footprints(testloader, batch_size, sz, gamma_c=0, iter_c=a.iter_c, **spatial)
    if a.spatial_solver == "hals":
        print("footprint KKT after the last step: max %.3e  median %.3e"
              % (float(dnmf.last_spatial_kkt.max()), float(dnmf.last_spatial_kkt.median())))
    if a.clean_footprints:
        before = (dnmf.fp.A > 0).reshape(-1, K).sum(0).tolist()
        fc = dnmf.clean_footprints()
        print("clean_footprints: %d of %d neurons cleaned" % (int(fc["ok"].sum()), K))
        for k in range(K):
            print("  neuron %2d: n_box %4d  n_kept %4d  n_parts %2d  (voxels > 0 before: %d)"
                  % (k, int(fc["n_box"][k]), int(fc["n_kept"][k]), int(fc["n_parts"][k]), before[k]))
    C = dnmf.C.cpu().numpy()
    corr = [np.corrcoef(C[k], dataset.traces[k])[0, 1] for k in range(K)]
    print("A_t", A_t.shape, "Y_i", Y_i.shape, "Y", Y.shape)
    print("trace correlation with ground truth: min %.3f  median %.3f" % (min(corr), float(np.median(corr))))
    if a.ar1:
        fitted, truth = dnmf.C.clone(), np.asarray(dataset.traces, np.float64)

        def median_corr_of(**kw):
            dnmf.C = fitted.clone()
            dnmf.update_footprints(testloader, batch_size, sz, gamma_c=0, iter_c=a.ar1, return_dense=False, **kw)
            X = dnmf.C.cpu().numpy().astype(np.float64)
            return float(np.median([np.corrcoef(X[k], truth[k])[0, 1] for k in range(K)]))

        hals = median_corr_of(solver='hals')
        base = torch.quantile(dnmf.C.float(), 0.08, dim=1).double().cpu()     # the HALS traces' own 8th percentile, per neuron
        ar1 = median_corr_of(solver='ar1', ar_g=float(np.exp(-0.3)), ar_penalty=a.ar_penalty, ar_baseline=base)
        info = dnmf.last_temporal_ar
        print("median trace correlation with ground truth after %d sweeps from the fitted C: 'hals' %.4f  'ar1' %.4f  (g = e^-0.3, "
              "penalty %g, baseline = the 8th percentile of the 'hals' traces; %d colours, F %.6e -> %.6e)"
              % (a.ar1, hals, ar1, a.ar_penalty, info["n_colours"], info["F"][0], info["F"][1]))
        dnmf.C = fitted
    if a.denoise:
        sz_list = [int(n) for n in sz]
        den = dnmf.denoise_movie(testloader, registered='linear')
        raw = dnmf.summary_images(testloader, registered='linear')["corr"]
        after = ExponentialFP.summary_images((den, sz_list))["corr"]
        print("denoise: median kept per patch %g of rank %d (%d patches, %d usable); peak of the corr image: raw registered %.3f  "
              "denoised %.3f" % (float(dnmf.last_denoise["kept"].float().median()), dnmf.last_denoise["lam"].shape[1],
                                 dnmf.last_denoise["kept"].numel(), int(dnmf.last_denoise["ok"].sum()),
                                 float(raw.nan_to_num(-1.0).max()), float(after.nan_to_num(-1.0).max())))
    if a.clean is not None:
        cleaned =dnmf.clean_traces(a.clean)[0].cpu().numpy().astype(np.float64)

        def median_corr(X):
            cc = []
            for k in range(K):
                ok = ~np.isnan(cleaned[k])        # the frames the clean-up keeps, for both
                cc.append(np.corrcoef(X[k][ok], np.asarray(dataset.traces[k])[ok])[0, 1] if ok.sum() > 2 else np.nan)
            return float(np.nanmedian(cc))

        print("median trace correlation with ground truth at %g fps: C %.3f  cleaned C %.3f  (outliers removed: %d, curves fitted: %d of %d)"
              % (a.clean, median_corr(C), median_corr(cleaned), int(dnmf.last_clean["n_outliers"].sum()),
                 int(dnmf.last_clean["fitted"].sum()), K))
    if a.dff:
        detrended = dnmf.detrend_traces(a.dff).cpu().numpy().astype(np.float64)
        print("median trace correlation with ground truth: C %.3f  C against its running baseline (window %d) %.3f"
              % (float(np.median(corr)), a.dff, float(np.median([np.corrcoef(detrended[k], dataset.traces[k])[0, 1] for k in range(K)]))))
    if a.deconvolve:
        c, s, info = dnmf.deconvolve()
        ok = info["ok"].cpu().numpy()
        fit = (info["baseline"][:, None] + c).cpu().numpy().astype(np.float64)
        truth = np.asarray(dataset.traces, np.float64)
        print("median trace correlation with ground truth: C %.3f  b + c %.3f;  median estimated decay %.3f (simulator: %.3f);  %d of %d traces treated"
              % (float(np.median([np.corrcoef(C[k], truth[k])[0, 1] for k in range(K) if ok[k]])),
                 float(np.median([np.corrcoef(fit[k], truth[k])[0, 1] for k in range(K) if ok[k]])),
                 float(np.nanmedian(info["g"].cpu().numpy())), float(np.exp(-0.3)), int(ok.sum()), K))
    if a.match:
        truth = np.asarray(dataset.traces, np.float64)
        matched = dnmf.match_traces(dataset.traces).cpu().numpy().astype(np.float64)

        def median_rms(X):
            return float(np.median(np.sqrt(np.mean((X - truth) ** 2, axis=1))))

        print("median RMS difference from ground truth: C %.4f  matched C %.4f  (median trace correlation %.3f; median scale %.3f, "
              "median quantile distance %.4f)"
              % (median_rms(C.astype(np.float64)), median_rms(matched), float(np.median(corr)),
                 float(dnmf.last_match["beta"][:, 0].median()), float(dnmf.last_match["distance"].median())))
    if a.evaluate:
        ev = dnmf.evaluate_components(testloader)
        np.set_printoptions(precision=2, suppress=True, linewidth=160)
        print("component evaluation over %d active frames each: r_values %s" % (ev["n_active"], ev["r_values"].cpu().numpy()))
        print("snr %s" % ev["snr"].cpu().numpy())
        print("keep %s  (%d of %d)" % (ev["keep"].int().cpu().numpy(), int(ev["keep"].sum()), K))
    if a.add:
        out = dnmf.add_components(testloader, a.add)
        np.set_printoptions(precision=3, suppress=True, linewidth=160)
        print("add: %d candidates, explained/energy %s" % (len(out["kept"]), (out["explained"] / out["energy"]).cpu().numpy()))
        print("kept %s" % out["kept"].int().cpu().numpy())
        print("K %d -> %d  (%d added)" % (K, out["K"], out["added"]))
        K = out["K"]
    if a.merge:
        out = dnmf.merge_components()
        off = out["pairs"][:, 0] != out["pairs"][:, 1]
        print("merge: %d candidate pairs, largest trace correlation %.3f, largest footprint overlap %.3f"
              % (int(off.sum()), float(out["corr"][off].nan_to_num(-1.0).max()) if bool(off.any()) else float("nan"),
                 float(out["overlap"][off].max()) if bool(off.any()) else float("nan")))
        print("groups %s" % out["groups"])
        print("K %d -> %d  (%d merged groups)" % (K, out["K"], out["merged"]))
    return corr


if __name__ == "__main__":
    main()
