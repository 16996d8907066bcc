"""Position initialiser: the part of the reference's ``Demix/MotionCorrect.py`` (a vendored copy of CaImAn / NoRMCorre
that nothing in the reference tree calls) that turns a 3-D video into per-frame neuron positions:

    mc = MotionCorrect(video, max_shifts=(6, 6, 1), strides=(24, 24, 1), overlaps=(8, 8, 1), is3D=True)
    mc.motion_correct_pwrigid(template=template)         # fills x_shifts_els, y_shifts_els, z_shifts_els
    positions = mc.apply_shifts_points(video, points)    # (K, 3, T): what DeformableNMF / a tracker starts from

Same constructor arguments, attribute names and method names as the reference class (``MotionCorrect.py:64-385``), limited
to what ``apply_shifts_points`` (``:351-371``) needs: the per-patch shifts of the 3-D piecewise-rigid pass
(``tile_and_correct_3d`` ``:1518-1608`` with the class default ``shifts_opencv=True``, ``upsample_factor_fft=10`` as
``tile_and_correct_wrapper`` ``:2029-2037`` hard-codes it).  The registration runs on the GPU (K8 ``dnmf_register_patches``:
matrix-multiply DFTs, no FFT library; ``csrc/register_patches.hip``).

``template=None`` runs the reference's rigid pre-pass first (``motion_correct_rigid`` ``:213-258`` ->
``motion_correct_batch_rigid`` ``:1770-1877``): the binned median of the video as the first template, every frame
registered to it and moved by its shift through the phases of its spectrum (``apply_shifts_dft``), the NaN-aware mean of the
moved frames as the template of the piecewise pass -- K8 ``dnmf_rigid_correct``.  ``motion_correct_rigid`` is also offered
on its own (``shifts_rig``, ``total_template_rig``, ``templates_rig``; the corrected movie in ``mc`` only with
``save_corrected=True``: it is as large as the video).

2-D videos (``is3D=False``, (T, X, Y); ``register_translation`` ``:801-1024``, ``tile_and_correct`` ``:1272-1418``) are
registered as one slice of the same kernels: ``motion_correct_pwrigid(template=...)`` fills ``x_shifts_els`` /
``y_shifts_els``.  (``apply_shifts_points`` is 3-D in the reference too.)

The piecewise-rigid corrected movie of a 3-D video (``tile_and_correct_3d`` ``:1639-1654``: the patch shifts resized to a
full-size field, the frame warped through it with a cubic B-spline, clipped to its range) runs on the GPU too (K9
``dnmf_apply_pwrigid``, ``csrc/apply_pwrigid.hip``): ``motion_correct_pwrigid`` with ``save_corrected=True`` fills ``mc_els``,
``templates_els`` and -- without a template -- ``total_template_els`` from it; ``apply_shifts_movie(video)`` applies the
stored (possibly edited) shifts to a video.  Deviations from the reference: the movie goes to ``mc_els``, not ``mc`` (the
reference's piecewise pass leaves ``mc`` to the rigid pass, ``:328`` is commented out); ``total_template_els`` is the 3-D
chunk template, where the reference's ``np.dstack`` (``motion_correct_batch_pwrigid`` ``:1970``) collapses a 3-D template
to (X, Y) -- a bug of the reference (its rigid path stacks correctly, ``:1860``); the warp sums in fp32 where skimage uses
float64 (within 1e-5 of the frame's range).

``gSig_filt`` (``high_pass_filter_space`` ``:1262-1270``, K22 ``dnmf_high_pass_frames``, ``csrc/high_pass.hip``): the shifts are
measured on a spatially high-pass-filtered copy of every frame -- a zero-sum Gaussian disc, reflected borders, slice by slice --
and applied to the unfiltered frame (``tile_and_correct_3d`` ``:1581-1587``, ``:1640-1641``): what registers a movie whose static
or slowly varying background outweighs its cells.  A given template is used as given (pass a filtered one); every template
this class makes is filtered before it is used (``:1825-1829``, ``:1863-1864``).  The reference's 3-D rigid branch raises with
``gSig_filt`` (``:1598-1600``); here, as an extension, the rigid pass measures on the filtered frames (K8) and moves the
ORIGINAL frames by K9 with every patch given the frame's rigid shift -- an interpolating move, as the reference's 2-D path
(``cv2.warpAffine``) makes.

Not offered (``NotImplementedError``): the 2-D piecewise-corrected movie (``cv2.resize`` + ``cv2.remap``), the 2-D rigid
correction (``cv2.warpAffine``), ``shifts_opencv=False`` (cubic resize of the shift field), memory-mapped files, ``dview``.

Parity: the 3-D piecewise path -- K8's patch shifts and K9's corrected movie and chunk template -- is pinned by the G11
fixtures (``tests/golden/make_golden_motion.py``: the reference module itself, run under a Python with scikit-image, with
a stub for cv2, which that path never calls).  The rest of the class is checked against ``oracle/motion_oracle.py``, a
numpy restatement of the same functions.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import ops

device = 'cuda'


def high_pass_filter_space(img_orig, gSig_filt):
    """Reference :1262-1270 on the GPU (K22): ``img_orig`` (X, Y) or (X, Y, Z) cast to float32 and correlated, slice by slice,
    with the zero-sum Gaussian disc of ``gSig_filt[0]`` (``ops.high_pass_taps``), borders reflected (cv2's BORDER_REFLECT).
    numpy in: float32 numpy out; a CUDA tensor in: a float32 CUDA tensor out."""
    t = img_orig if torch.is_tensor(img_orig) else torch.from_numpy(np.ascontiguousarray(np.asarray(img_orig, dtype=np.float32)))
    if t.dim() not in (2, 3):
        raise ValueError(f"high_pass_filter_space: an image is (X, Y) or (X, Y, Z), got {tuple(t.shape)}")
    sz = [int(v) for v in t.shape] + [1] * (3 - t.dim())
    out = ops.high_pass_frames(t.to(device, torch.float32).reshape(1, -1).contiguous(), sz, gSig_filt).view(*t.shape)
    return out if torch.is_tensor(img_orig) else out.cpu().numpy()


class MotionCorrect(object):
    def __init__(self, video, min_mov=None, dview=None, max_shifts=(6, 6, 1), niter_rig=1, splits_rig=1,
                 num_splits_to_process_rig=None, strides=(96, 96, 1), overlaps=(32, 32, 1), splits_els=1,
                 num_splits_to_process_els=None, upsample_factor_grid=4, max_deviation_rigid=3, shifts_opencv=True,
                 nonneg_movie=True, gSig_filt=None, use_cuda=False, border_nan=True, pw_rigid=False, num_frames_split=80,
                 var_name_hdf5='mov', is3D=True, indices=(slice(None), slice(None)), save_corrected=False):
        ops._lib.load()   # fail here, loudly, if the HIP library is not built
        if not shifts_opencv:
            raise NotImplementedError("MotionCorrect: shifts_opencv=False (cubic resize of the shift field) is not built")
        if dview is not None:
            raise NotImplementedError("MotionCorrect: dview (a process pool) is not built; the GPU walks the video in pieces of its own")
        if gSig_filt is not None:
            ops.high_pass_taps(gSig_filt)     # ValueError for an entry <= 0 or not finite
            gSig_filt = tuple(float(v) for v in gSig_filt) if hasattr(gSig_filt, '__len__') else (float(gSig_filt),) * 2
        self.gSig_filt = gSig_filt
        if type(video) is not list:
            video = [video]
        self.video = video
        self.is3D = bool(is3D)
        self.max_shifts = tuple(int(v) for v in max_shifts)
        self.strides = tuple(int(v) for v in strides)
        self.overlaps = tuple(int(v) for v in overlaps)
        nd = 3 if self.is3D else 2
        if not self.is3D:
            # 2-D videos (T, X, Y) -- register_translation :801-1024, tile_and_correct :1272-1418 -- run as one slice of the
            # 3-D kernels: a third axis of one voxel has no window and a zero shift.  (A 2-D call may still pass the 3-entry
            # defaults of this class: their third entries are dropped.)
            self.max_shifts, self.strides, self.overlaps = self.max_shifts[:2], self.strides[:2], self.overlaps[:2]
        if not (len(self.max_shifts) == len(self.strides) == len(self.overlaps) == nd):
            raise ValueError(f"MotionCorrect: max_shifts, strides and overlaps need {nd} entries")
        self.max_deviation_rigid = int(max_deviation_rigid)
        self.upsample_factor_grid = upsample_factor_grid
        self.shifts_opencv = True
        self.min_mov = min_mov
        self.nonneg_movie = nonneg_movie
        if border_nan not in (True, False, 'min', 'copy'):
            raise ValueError(f"MotionCorrect: border_nan {border_nan!r}")
        self.border_nan = border_nan
        self.niter_rig = int(niter_rig)
        if splits_rig != 1 or splits_els != 1 or num_splits_to_process_rig is not None or num_splits_to_process_els is not None:
            raise NotImplementedError("MotionCorrect: splits (chunks for a process pool) are not built; the GPU walks the video "
                                      "in pieces of its own")
        self.save_corrected = bool(save_corrected)
        self.pw_rigid = bool(pw_rigid)
        self.upsample_factor_fft = 10     # tile_and_correct_wrapper :2029-2037

    def _p3(self):
        """strides, overlaps, max_shifts with three entries (one slice for a 2-D video: window 1, no shift)."""
        if self.is3D:
            return self.strides, self.overlaps, self.max_shifts
        return self.strides + (1,), self.overlaps + (0,), self.max_shifts + (0,)

    def _frames(self, video):
        """(T, X, Y, Z) -- (T, X, Y) for is3D=False -- numpy / torch -> (T, P) fp32 CUDA rows and the volume size (Z = 1)."""
        v = torch.as_tensor(np.asarray(video) if not torch.is_tensor(video) else video)
        if not self.is3D and v.dim() == 3:
            v = v[..., None]
        if v.dim() != 4 or (not self.is3D and v.shape[3] != 1):
            raise ValueError(f"MotionCorrect: a video is (T, X, Y, Z) (is3D) or (T, X, Y), got {tuple(v.shape)}")
        sz = [int(s) for s in v.shape[1:]]
        return v.to(device, torch.float32).reshape(v.shape[0], -1).contiguous(), sz

    def _filtered(self, frames, sz):
        """Pieces (f0, rows) of the frames a registration reads: the rows themselves, or with ``gSig_filt`` their high-pass (K22) in
        pieces of at most 1 GiB."""
        T, P = frames.shape
        if self.gSig_filt is None:
            yield 0, frames
            return
        step = max(1, min(T, (1 << 30) // (4 * P)))
        for f0 in range(0, T, step):
            yield f0, ops.high_pass_frames(frames[f0:f0 + step], sz, self.gSig_filt)

    def motion_correct(self, template=None):
        """Reference :176-211."""
        if self.min_mov is None:
            self.min_mov = min(float(torch.as_tensor(v).min()) for v in self.video)     # (:193-195: of the first video)
        if self.pw_rigid:
            self.motion_correct_pwrigid(template=template)
            b0 = np.ceil(np.max([np.max(np.abs(self.x_shifts_els)), np.max(np.abs(self.y_shifts_els))] +
                                ([np.max(np.abs(self.z_shifts_els))] if self.is3D else [])))
        else:
            self.motion_correct_rigid(template=template)
            b0 = np.ceil(np.max(np.abs(self.shifts_rig)))
        self.border_to_0 = int(b0)
        return self

    @staticmethod
    def _bin_median_3d(frames, window=10):
        """bin_median_3d :464-494 on (T, P) rows: mean over groups of frames (group j = frames j, j + num_windows, ...: the
        reference's reshape), NaN-aware median over the groups (mean of the two middle values for an even count)."""
        T = frames.shape[0]
        window = min(window, T)
        nw = T // window
        bins = frames[:nw * window].view(window, nw, -1).nanmean(0)          # (nw, P)
        srt = bins.sort(0).values                                            # NaNs last
        cnt = (~torch.isnan(bins)).sum(0).clamp(min=1)
        lo = srt.gather(0, ((cnt - 1) // 2)[None])[0]
        hi = srt.gather(0, (cnt // 2)[None])[0]
        return 0.5 * (lo + hi)

    def motion_correct_rigid(self, template=None):
        """Reference :213-258 -> motion_correct_batch_rigid :1770-1877 (3-D, one chunk): fills ``total_template_rig``,
        ``templates_rig``, ``shifts_rig`` (one (x, y, z) tuple per frame, the registration's shift with its sign flipped,
        :1574) and -- only with ``save_corrected=True`` -- ``mc`` (one (X, Y, Z, T) array per video)."""
        if not self.is3D:
            # (the reference moves 2-D frames with cv2.warpAffine when shifts_opencv is set, :1349-1354, and its own 2-D start
            # without a template calls a method numpy arrays do not have, :1828)
            raise NotImplementedError("MotionCorrect.motion_correct_rigid: the 2-D rigid correction (cv2.warpAffine) is not built; "
                                      "2-D videos: motion_correct_pwrigid(template=...)")
        self.total_template_rig = template
        self.templates_rig, self.shifts_rig, self.mc = [], [], []
        for video_cur in self.video:
            frames, sz = self._frames(video_cur)
            if self.min_mov is None:
                self.min_mov = float(frames.min())
            if self.gSig_filt is not None:
                rigid, tmpl, moved = self._rigid_filtered(frames, sz)
            elif self.total_template_rig is None:
                tmpl = self._bin_median_3d(frames)                           # :1826
            else:
                tmpl = torch.as_tensor(np.asarray(self.total_template_rig) if not torch.is_tensor(self.total_template_rig)
                                       else self.total_template_rig).to(device, torch.float32).reshape(-1)
            add = float(np.float32(-self.min_mov))                           # (:2122: passed on as a float32)
            step = max(1, min(frames.shape[0], (1 << 30) // (4 * frames.shape[1]))) if self.save_corrected else frames.shape[0]
            for it in range(max(1, self.niter_rig) if self.gSig_filt is None else 0):
                last = it == max(1, self.niter_rig) - 1
                tsum = tcount = None
                parts, moved = [], []
                for f0 in range(0, frames.shape[0], step):
                    r, out, tsum, tcount = ops.rigid_correct(frames[f0:f0 + step], tmpl, sz, self.max_shifts, self.upsample_factor_fft,
                                                             add_to_movie=add, border_nan=self.border_nan,
                                                             want_frames=self.save_corrected and last, tsum=tsum, tcount=tcount)
                    parts.append(r)
                    if out is not None:
                        moved.append(out.cpu())
                rigid = torch.cat(parts)
                new_temp = tsum / tcount                                     # nanmean :2057 (0 / 0: NaN)
                new_temp = torch.where(torch.isnan(new_temp), new_temp[~torch.isnan(new_temp)].min(), new_temp)   # :2058
                tmpl = new_temp
                moved = [torch.cat(moved)] if moved else []
            if template is None:
                self.total_template_rig = tmpl.view(*sz).cpu().numpy()
            self.templates_rig.append(tmpl.view(*sz).cpu().numpy())
            self.shifts_rig += [tuple(float(-v) for v in row) for row in rigid.cpu().numpy()]
            if moved:
                self.mc.append(moved[0].view(-1, *sz).permute(1, 2, 3, 0).numpy())

    def _rigid_filtered(self, frames, sz):
        """The rigid pass with ``gSig_filt`` (an extension: the reference's 3-D rigid branch raises, :1598-1600): the first template
        is the binned median of the FILTERED movie (:1825-1829) or the one given, as given; K8 measures every frame's shift on the
        filtered rows (nothing filtered is moved); K9 moves the ORIGINAL rows, every patch given the frame's rigid shift in the
        sign convention of ``x/y/z_shifts_els``; the new template is the NaN-aware mean of the moved originals, NaN -> min
        (:2057-2058), then filtered (:1863-1864).  -> (shifts (T, 3) as K8 returns them, the last template (P,), [moved rows on
        the host] with ``save_corrected``)."""
        T, P = frames.shape
        strides, overlaps, max_shifts = self._p3()
        NP = len(ops.patch_grid(sz, strides, overlaps)[1])
        if self.total_template_rig is None:
            pieces = [rows for _, rows in self._filtered(frames, sz)]
            tmpl = self._bin_median_3d(pieces[0] if len(pieces) == 1 else torch.cat(pieces))
            del pieces
        else:
            tmpl = torch.as_tensor(np.asarray(self.total_template_rig) if not torch.is_tensor(self.total_template_rig)
                                   else self.total_template_rig).to(device, torch.float32).reshape(-1)
        add = float(np.float32(-self.min_mov))
        step = max(1, min(T, (1 << 30) // (4 * P)))
        niter = max(1, self.niter_rig)
        for it in range(niter):
            keep = self.save_corrected and it == niter - 1
            tsum = tcount = None
            parts, moved = [], []
            for f0, rows in self._filtered(frames, sz):
                r = ops.rigid_correct(rows, tmpl, sz, self.max_shifts, self.upsample_factor_fft, add_to_movie=add,
                                      border_nan=self.border_nan, want_frames=False)[0]
                parts.append(r)
                del rows
                for g0 in range(0, r.shape[0], step):
                    table = self._rigid_table(r[g0:g0 + step], NP)
                    out, tsum, tcount = ops.apply_pwrigid(frames[f0 + g0:f0 + g0 + step], table, sz, strides, overlaps,
                                                          add_to_movie=add, tsum=tsum, tcount=tcount)
                    if keep:
                        moved.append(out.cpu())
            new_temp = tsum / tcount                                         # nanmean :2057 (0 / 0: NaN)
            new_temp = torch.where(torch.isnan(new_temp), new_temp[~torch.isnan(new_temp)].min(), new_temp)   # :2058
            tmpl = ops.high_pass_frames(new_temp.view(1, P), sz, self.gSig_filt).view(P)     # :1863-1864
        return torch.cat(parts), tmpl, ([torch.cat(moved)] if moved else [])

    def _rigid_table(self, rigid, NP):
        """(B, 3) rigid shifts as K8 returns them -> the (B, NP, 3) table K9 takes: every patch the frame's shift, signs as in
        ``x/y/z_shifts_els`` (-x, -y, +z)."""
        sign = torch.tensor([-1.0, -1.0, 1.0], dtype=torch.float32, device=rigid.device)
        return (rigid * sign)[:, None, :].expand(-1, NP, -1).contiguous()

    def motion_correct_pwrigid(self, template=None, show_template=False):
        """Reference :260-328: fills ``x_shifts_els``, ``y_shifts_els``, ``z_shifts_els`` (one (NP,) array per frame),
        ``shifts_rig`` (the rigid shift of every frame), ``coord_shifts_els`` (the patch grid indices) and
        ``total_template_els``.  3-D videos with ``save_corrected=True`` also get the piecewise-rigid corrected movie (K9):
        ``mc_els`` (one (X, Y, Z, T) float32 array per video; ``mc`` keeps the rigid pass's movie, as the reference leaves
        it, :328), ``templates_els`` (one (X, Y, Z) chunk template per video, the NaN-aware mean of the corrected frames,
        :2057-2058) and, when ``template`` is None, ``total_template_els`` = that template.  With ``gSig_filt`` the shifts are
        measured on the high-pass-filtered frames (K22) against the template as given -- pass a filtered one -- and K9 moves the
        original frames (:1640-1641); without a template the pass registers against the filtered ``total_template_rig``, and
        ``total_template_els`` is that filtered image unless a corrected movie is made."""
        self.x_shifts_els, self.y_shifts_els = [], []
        if self.is3D:
            self.z_shifts_els = []
        self.coord_shifts_els = []
        corrected = self.save_corrected and self.is3D
        if corrected:
            self.mc_els, self.templates_els = [], []
        strides, overlaps, max_shifts = self._p3()
        for video_cur in self.video:
            frames, sz = self._frames(video_cur)
            if self.min_mov is None:
                self.min_mov = float(frames.min())           # :196-199
            if template is None:
                self.motion_correct_rigid()                  # :298-301 (every video of the list, as the reference does)
                tmpl = torch.from_numpy(np.ascontiguousarray(self.total_template_rig)).to(device, torch.float32).reshape(-1)
            else:
                tmpl = torch.as_tensor(np.asarray(template) if not torch.is_tensor(template) else template).to(
                    device, torch.float32).reshape(-1)
            self.total_template_els = tmpl.view(*sz) if self.is3D else tmpl.view(*sz[:2])
            # (with gSig_filt the shifts are measured on the filtered rows, :1581-1587; frames are independent)
            parts = [ops.register_patches(rows, tmpl, sz, strides, overlaps, max_shifts, self.max_deviation_rigid,
                                          self.upsample_factor_fft, add_to_movie=-self.min_mov)[1]
                     for _, rows in self._filtered(frames, sz)]
            patch = parts[0] if len(parts) == 1 else torch.cat(parts)
            dims, starts = ops.patch_grid(sz, strides, overlaps)
            nd = 3 if self.is3D else 2
            grid = [tuple(int(v) for v in np.unravel_index(q, dims))[:nd] for q in range(len(starts))]
            p = patch.cpu().numpy()
            for t in range(p.shape[0]):
                self.x_shifts_els.append(p[t, :, 0].copy())
                self.y_shifts_els.append(p[t, :, 1].copy())
                if self.is3D:
                    self.z_shifts_els.append(p[t, :, 2].copy())
                self.coord_shifts_els.append(grid)
            self._patch_shifts = patch                       # (T, NP, 3) on the GPU, for apply_shifts_points
            if corrected:
                movie, new_temp = self._corrected_movie(frames, sz, patch)
                self.mc_els.append(movie)
                self.templates_els.append(new_temp.cpu().numpy())
                if template is None:
                    self.total_template_els = new_temp

    def _corrected_movie(self, frames, sz, patch):
        """K9 on (T, P) rows and their (T, NP, 3) shifts, in pieces of at most 1 GiB of output: (the corrected movie as
        (X, Y, Z, T) float32 numpy, its chunk template (X, Y, Z) on the GPU -- nanmean over the frames, NaN -> nanmin)."""
        strides, overlaps, _ = self._p3()
        add = float(np.float32(-self.min_mov))               # (:2122: passed on as a float32)
        T, P = frames.shape
        step = max(1, min(T, (1 << 30) // (4 * P)))
        tsum = tcount = None
        moved = []
        for f0 in range(0, T, step):
            out, tsum, tcount = ops.apply_pwrigid(frames[f0:f0 + step], patch[f0:f0 + step].contiguous(), sz, strides, overlaps,
                                                  add_to_movie=add, tsum=tsum, tcount=tcount)
            moved.append(out.cpu())
        new_temp = tsum / tcount                             # nanmean :2057 (0 / 0: NaN)
        new_temp = torch.where(torch.isnan(new_temp), new_temp[~torch.isnan(new_temp)].min(), new_temp)   # :2058
        return torch.cat(moved).view(-1, *sz).permute(1, 2, 3, 0).numpy(), new_temp.view(*sz)

    def apply_shifts_movie(self, video):
        """The video (T, X, Y, Z) moved by the STORED piecewise shifts ``x/y/z_shifts_els`` (a caller may have edited them):
        tile_and_correct_3d :1639-1654 per frame, with add_to_movie = -min_mov.  (X, Y, Z, T) float32 numpy, like ``mc``."""
        if not self.is3D:
            raise NotImplementedError("MotionCorrect.apply_shifts_movie: the 2-D piecewise-corrected movie (cv2.resize + "
                                      "cv2.remap, reference :1405-1410) is not built")
        frames, sz = self._frames(video)
        if self.min_mov is None:
            self.min_mov = float(frames.min())
        movie, _ = self._corrected_movie(frames, sz, self._shift_table(frames.shape[0]))
        return movie

    def _centers(self, sz):
        _, starts = ops.patch_grid(sz, self.strides, self.overlaps)
        return starts.astype(np.float64) + np.array(self.strides, dtype=np.float64) / 2     # :366

    def _shift_table(self, T):
        """(T, NP, 3) fp32 CUDA from the lists (a caller may have edited them)."""
        sh = np.stack([np.stack(self.x_shifts_els[:T]), np.stack(self.y_shifts_els[:T]), np.stack(self.z_shifts_els[:T])], 2)
        return torch.from_numpy(sh.astype(np.float32)).to(device)

    def summary_images(self, video=None, neighbours='full'):
        """The summary images (K18, ``ExponentialFP.summary_images``) of a (T, X, Y, Z) ``video`` or, without one, of the stored
        corrected movie -- ``mc_els`` when the piecewise pass kept one, else ``mc`` (``save_corrected=True``; several videos
        count as one movie): a dict ``mean / std / max / corr`` of (X, Y, Z) float64 numpy images (CUDA tensors for a CUDA
        ``video``).  The stored movie goes to the GPU in pieces of at most 1 GiB.  Voxels the correction left NaN in some
        frame are NaN."""
        from .dNMF import ExponentialFP
        if video is not None:
            return ExponentialFP.summary_images(video, neighbours=neighbours)
        movies = getattr(self, "mc_els", None) or getattr(self, "mc", None)
        if not movies:
            raise ValueError("MotionCorrect.summary_images: no video given and no corrected movie stored; construct with "
                             "save_corrected=True and call motion_correct() first")
        sz = [int(n) for n in movies[0].shape[:3]]
        P = sz[0] * sz[1] * sz[2]
        limit = max(1, (1 << 30) // (4 * P))
        pieces = [(m, s, min(m.shape[3], s + limit)) for m in movies for s in range(0, m.shape[3], limit)]
        state = ops.summary_images_state(sz, max(e - s for _, s, e in pieces), neighbours=neighbours, device=device)
        for n, (m, s, e) in enumerate(pieces):
            rows = torch.from_numpy(np.ascontiguousarray(np.moveaxis(m[..., s:e], 3, 0))).to(device, torch.float32).reshape(e - s, P)
            images, state = ops.summary_images(rows, sz, neighbours=neighbours, state=state, first=n == 0, finish=n == len(pieces) - 1)
        return {k: v.cpu().numpy() for k, v in images.items()}

    def _stored_pieces(self, who):
        """``(pieces, sz)`` of the stored corrected movie -- ``mc_els`` when the piecewise pass kept one, else ``mc``; several
        videos count as one movie: ``pieces()`` yields it as (rows, P) fp32 CUDA tensors of at most 1 GiB, in order."""
        movies = getattr(self, "mc_els", None) or getattr(self, "mc", None)
        if not movies:
            raise ValueError(f"MotionCorrect.{who}: no video given and no corrected movie stored; construct with "
                             "save_corrected=True and call motion_correct() first")
        sz = [int(n) for n in movies[0].shape[:3]]
        P = sz[0] * sz[1] * sz[2]
        limit = max(1, (1 << 30) // (4 * P))

        def pieces():
            for m in movies:
                for s in range(0, m.shape[3], limit):
                    e = min(m.shape[3], s + limit)
                    yield torch.from_numpy(np.ascontiguousarray(np.moveaxis(m[..., s:e], 3, 0))).to(device, torch.float32).reshape(e - s, P)
        return pieces, sz

    def robust_images(self, video=None, **kw):
        """The order-statistic images (K30, ``ExponentialFP.robust_images``; ``kw``: ``percentiles``, ``noise``) of a
        (T, X, Y, Z) ``video`` or, without one, of the stored corrected movie, as ``summary_images`` takes it: a dict
        ``median / max / mad / noise / pnr / n / percentile`` of (X, Y, Z) numpy images (CUDA tensors for a CUDA ``video``).
        The stored movie goes to the GPU in pieces of at most 1 GiB, once per pass of the selection.  Samples the
        correction left NaN are left out of their voxel's statistics (``n`` counts the others)."""
        from .dNMF import ExponentialFP, _images_to_numpy
        if video is not None:
            return ExponentialFP.robust_images(video, **kw)
        pieces, sz = self._stored_pieces("robust_images")
        return _images_to_numpy(ops.robust_images(pieces, sz, **kw))

    def dff_movie(self, video=None, **kw):
        """The dF/F movie (K31, ``ExponentialFP.dff_movie``; ``kw``: ``window``, ``stride``, ``percentile``, ``mode``, ``offset``,
        ``min_samples``) of a (T, X, Y, Z) ``video`` or, without one, of the stored corrected movie, as ``robust_images`` takes
        it -> ``(movie, info)``: numpy float32 (T, X, Y, Z) and the knots of the running baseline (CUDA rows (T, P) for a CUDA
        ``video``).  The stored movie is held on the GPU whole while the call runs, as the movie that comes back is; the kernels
        take it in pieces of at most 1 GiB.  Samples the correction left NaN are left out of their windows and stay NaN in the
        movie."""
        from .dNMF import ExponentialFP
        if video is not None:
            return ExponentialFP.dff_movie(video, **kw)
        pieces, sz = self._stored_pieces("dff_movie")
        percentile = float(kw.pop("percentile", 8.0))
        if not 0.0 <= percentile <= 100.0:
            raise ValueError(f"MotionCorrect.dff_movie: percentile must lie in [0, 100], got {percentile!r}")
        held = list(pieces())
        edges = np.cumsum([0] + [p.shape[0] for p in held])

        def rows_of(r0, r1):
            first, last = np.searchsorted(edges, r0, side="right") - 1, np.searchsorted(edges, r1, side="left") - 1
            if first == last:
                return held[first][r0 - edges[first]:r1 - edges[first]]
            return torch.cat([held[i][max(r0, edges[i]) - edges[i]:min(r1, edges[i + 1]) - edges[i]] for i in range(first, last + 1)])
        T = int(edges[-1])
        movie, info = ops.dff_rows(rows_of, T, sz, kw.pop("window"), kw.pop("stride", None), percentile / 100.0, **kw)
        info = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in info.items()}
        return movie.cpu().numpy().reshape(T, *sz), info

    def denoise_movie(self, video=None, **kw):
        """The corrected movie denoised by local low-rank approximation (K34, ``ExponentialFP.denoise_movie``; ``kw``: ``patch``,
        ``overlap``, ``rank``, ``keep``, ``threshold``, ``iters``, ``scale``) -> ``(movie, info)``: of an (X, Y, Z, T) ``video``, the
        layout of ``mc``, or, without one, of the stored corrected movie (``save_corrected=True``; several videos count as one
        movie), a float32 numpy (X, Y, Z, T) movie and the numpy ``kept``, ``lam``, ``ok``, ``explained``, ``U``, ``Q`` and ``plan``.
        The stored movie is held on the GPU whole while the call runs; the kernels take it in pieces of at most 1 GiB.  A patch
        that holds a sample the correction left NaN is left out, and its voxels come back as they are where no other patch covers
        them."""
        from .dNMF import ExponentialFP, _denoise_rows
        if video is not None:
            return ExponentialFP.denoise_movie(video, **kw)
        pieces, sz = self._stored_pieces("denoise_movie")
        held = list(pieces())
        edges = np.cumsum([0] + [p.shape[0] for p in held])

        def rows_of(r0, r1):
            first, last = np.searchsorted(edges, r0, side="right") - 1, np.searchsorted(edges, r1, side="left") - 1
            if first == last:
                return held[first][r0 - edges[first]:r1 - edges[first]]
            return torch.cat([held[i][max(r0, edges[i]) - edges[i]:min(r1, edges[i + 1]) - edges[i]] for i in range(first, last + 1)])
        T = int(edges[-1])
        movie, info = _denoise_rows(rows_of, T, sz, kw.pop("scale", 'noise'), **kw)
        info = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in info.items()}
        return movie.view(T, *sz).permute(1, 2, 3, 0).cpu().numpy(), info

    def detect_points(self, K, shape_std=3, **kw):
        """The (n, 3) centres of the up to K neurons found in the template -- ``total_template_els`` when the piecewise pass
        made one, else ``total_template_rig`` -- by ``ExponentialFP.detect_positions`` (K14; ``kw``: ``min_distance``,
        ``threshold``, ``background``): the ``points`` ``apply_shifts_points`` takes, float64 numpy, brightest first.  The
        reference has no counterpart (its real data comes with annotated positions).  With ``gSig_filt`` and ``template=None``
        the stored template is a high-pass-filtered image (zero mean, negative around every cell) unless a corrected movie was
        made; pass ``background=0`` or search a summary image instead.

        ``image`` (keyword, default ``'template'``: the above, unchanged): ``'corr'``, ``'max'`` or ``'std'`` search that summary
        image of the stored corrected movie (``summary_images()``, K18; needs ``save_corrected=True``) -- the template averages
        over time and hides neurons that are dim on average but active; ``'temporal_median'`` and ``'pnr'`` search that image
        of ``robust_images()`` (K30) and ``'corr_pnr'`` the product of K18's ``corr`` and ``pnr``, the usual seed image: pnr
        shows an active cell however narrow and however dark its surroundings, where ``max`` and ``std`` show what is bright
        and noisy (the temporal median is not called ``'median'``: that spelling stays an error, as it has been); an
        (X, Y, Z) array is searched as given.  NaNs (the
        border strips the correction leaves, voxels without a valid neighbour) are replaced by the image's finite minimum,
        as the template's are."""
        if not self.is3D:
            raise NotImplementedError("MotionCorrect.detect_points is a 3-D function like apply_shifts_points; register 2-D "
                                      "videos as (T, X, Y, 1) with is3D=True")
        image = kw.pop("image", "template")
        from .dNMF import ExponentialFP
        if not isinstance(image, str) or image != "template":
            if isinstance(image, str):
                if image not in ("corr", "max", "std", "temporal_median", "pnr", "corr_pnr"):
                    raise ValueError(f"MotionCorrect.detect_points: image must be 'template', 'corr', 'max', 'std', "
                                     f"'temporal_median', 'pnr', 'corr_pnr' or an (X, Y, Z) array, got {image!r}")
                if image in ("corr", "max", "std"):
                    img = self.summary_images()[image]
                elif image == "corr_pnr":
                    img = self.summary_images()["corr"] * self.robust_images()["pnr"]
                else:
                    img = self.robust_images()["median" if image == "temporal_median" else image]
            else:
                img = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
                if img.ndim != 3:
                    raise ValueError(f"MotionCorrect.detect_points: an image is (X, Y, Z), got {img.shape}")
            img = np.array(img, dtype=np.float64)
            finite = np.isfinite(img)
            if not finite.any():
                raise ValueError("MotionCorrect.detect_points: the image has no finite voxel")
            img[~finite] = img[finite].min()
            pos, _ = ExponentialFP.detect_positions(img, K, shape_std=shape_std, **kw)
            return pos[np.isfinite(pos).all(1)].astype(np.float64)
        tmpl = getattr(self, "total_template_els", None)
        if tmpl is None:
            tmpl = getattr(self, "total_template_rig", None)
        if tmpl is None:
            raise ValueError("MotionCorrect.detect_points: no template yet, call motion_correct() first")
        tmpl = tmpl if torch.is_tensor(tmpl) else np.asarray(tmpl)
        pos, _ = ExponentialFP.detect_positions(tmpl, K, shape_std=shape_std, **kw)
        pos = pos.cpu().numpy() if torch.is_tensor(pos) else pos
        return pos[np.isfinite(pos).all(1)].astype(np.float64)

    def apply_shifts_points(self, video, points):
        """Reference :351-371: ``P_T`` (K, 3, T) float64 numpy -- point k in frame t, moved by the shifts of the patch whose
        centre is nearest to it, relative to frame 0."""
        if not self.is3D:
            raise NotImplementedError("MotionCorrect.apply_shifts_points is a 3-D function (reference :351-371: z_shifts_els, "
                                      "sliding_window_3d); register 2-D videos as (T, X, Y, 1) with is3D=True")
        v = np.asarray(video.shape) if hasattr(video, "shape") else None
        T, sz = int(v[0]), [int(s) for s in v[1:]]
        pts = torch.as_tensor(np.asarray(points)).to(device, torch.float32).contiguous()
        centers = torch.from_numpy(self._centers(sz)).to(device, torch.float32).contiguous()
        out = ops.apply_shifts_points(pts, self._shift_table(T), centers)
        return out.double().cpu().numpy()

    def track_points(self, video, points, search=None, shape_std=3, **kw):
        """``points`` (K,3) followed through ``video`` (T, X, Y, Z) by ``ExponentialFP.track_positions`` (K15): ``(P_T (K,3,T)
        float64, amplitudes (K,T))``, numpy.  The search of every frame is centred on ``apply_shifts_points(video, points)``
        when piecewise shifts are stored -- the patch grid's coarse track, refined per neuron -- else on the points
        themselves; ``search`` defaults to ``max_shifts``; ``kw``: ``threshold``, ``background``, ``exclude``.  A neuron within
        about 2 shape_std of a brighter one can be captured by it: ``search`` is the guard, ``exclude=R`` (K15x) the remedy.  The reference has no counterpart."""
        if not self.is3D:
            raise NotImplementedError("MotionCorrect.track_points is a 3-D function like apply_shifts_points; register 2-D "
                                      "videos as (T, X, Y, 1) with is3D=True")
        from .dNMF import ExponentialFP
        pts = np.asarray(points.cpu() if torch.is_tensor(points) else points, dtype=np.float64)
        predict = self.apply_shifts_points(video, pts) if getattr(self, "x_shifts_els", None) else None
        search = self.max_shifts if search is None else search
        pos, amp = ExponentialFP.track_positions(video, pts, shape_std=shape_std, search=search, predict=predict, **kw)
        if torch.is_tensor(pos):
            pos, amp = pos.cpu().numpy(), amp.cpu().numpy()
        return pos, amp

    def apply_shifts_frame(self, video, points, t):
        """Reference :330-349: the points moved by frame t's shifts (no reference frame, all three signs +)."""
        if not self.is3D:
            raise NotImplementedError("MotionCorrect.apply_shifts_frame is a 3-D function (reference :330-349)")
        from scipy.spatial import distance
        v = np.asarray(video.shape)
        sz = [int(s) for s in v[1:]]
        pts = np.asarray(points, dtype=np.float64)
        idx = distance.cdist(self._centers(sz), pts).argmin(0)
        A = pts.copy()
        A[:, 0] += np.asarray(self.x_shifts_els[t], dtype=np.float32)[idx]
        A[:, 1] += np.asarray(self.y_shifts_els[t], dtype=np.float32)[idx]
        A[:, 2] += np.asarray(self.z_shifts_els[t], dtype=np.float32)[idx]
        return A

    def get_params(self):
        return {'max_shifts': self.max_shifts, 'strides': self.strides, 'overlaps': self.overlaps,
                'upsample_factor_grid': self.upsample_factor_grid, 'max_deviation_rigid': self.max_deviation_rigid,
                'shifts_opencv': self.shifts_opencv, 'nonneg_movie': self.nonneg_movie, 'border_nan': self.border_nan,
                'is3D': self.is3D, 'gSig_filt': self.gSig_filt}
