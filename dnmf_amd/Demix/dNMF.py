"""Deformable NMF demixing on MI355X: the Python surface of the reference's ``Demix/dNMF.py``
(``ExponentialFP``, ``DeformableNMF``, ``SimulatedVideoDataset``) on hand-written HIP kernels.

The classes keep the reference's constructor arguments, attributes and method signatures so that its
``demo.py`` runs against this module unchanged (``from Demix.dNMF import ...`` resolves to this file
through the ``Demix`` package at the repository root).  What is different is underneath:

* ``ExponentialFP.forward`` (reference ``Demix/dNMF.py:53-62``) calls K1 ``dnmf_warp_gather`` for the
  materialised ``A_t`` / ``grid`` and the fused path (``dnmf_recon_image`` + K2 ``dnmf_warp_recon_grad``)
  for ``A_tC``; ``A_tC`` carries an autograd node whose backward is K2 again, so
  ``F.mse_loss(A_tC, batch).backward()`` deposits ``beta.grad`` like the reference.
* ``DeformableNMF.update_motion`` (``:181-194``) runs one fused K2 launch per mini-batch and hands
  ``beta.grad`` to the caller's optimiser; it never materialises the K warped footprints.
* ``DeformableNMF.update_footprints`` (``:163-179``) computes the per-frame Gram matrices and right-hand
  sides once with K3 ``dnmf_warp_gram_rhs`` (fp32 MFMA) and iterates the multiplicative update with K4
  ``dnmf_mu_temporal``; the reference recomputes both contractions in every iteration from a float64
  ``A_t`` of all frames.

There is no CPU fallback: without ``libdnmf_hip.so`` and a GPU these classes raise.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import Dataset

from .. import ops, sharding
from ..WUtils import Simulator

device = 'cuda'

# update_footprints returns the reference's dense (X,Y,Z,K,T) float64 A_t only below this many bytes
DENSE_RETURN_LIMIT = 1 << 31
# update_motion keeps the reconstruction images of all T frames resident below this many bytes
LISTS_BOXFRAC_LIMIT = 6.0   # 'auto' takes K3n below this mean number of footprint boxes per voxel
LISTS_MAX_K = 256           # neurons the neuron-list kernels (K3n, list reconstruction, list K5 / K6) hold
RECON_CACHE_LIMIT = 64 << 30
K2_MAX_FRAMES = 32768       # frames per K2 launch (they ride on gridDim.y)
STAGE_LIMIT = 96 << 30      # a host loader's frames are staged on the GPU once per pass below this many bytes
GN_CHUNK_BYTES = 1 << 30    # update_motion(solver='gn') builds the reconstruction images of this many bytes of frames at a time


def _images_to_numpy(images):
    """A dict of CUDA images, one level of nesting allowed, as numpy."""
    return {k: _images_to_numpy(v) if isinstance(v, dict) else v.cpu().numpy() for k, v in images.items()}


def _sz_list(sz):
    return [int(s) for s in (sz.tolist() if isinstance(sz, torch.Tensor) else sz)]


def _denoise_rows(rows_of, T, sz, scale='noise', **kw):
    """K34 on a movie of ``T`` frames that ``rows_of(r0, r1)`` serves as fp32 CUDA rows in time order: the centre is K18's mean,
    the scale K30's noise (``'noise'``), ones (``None``) or an (X, Y, Z) image -> ``ops.lowrank_denoise``'s (movie, info)."""
    P = sz[0] * sz[1] * sz[2]
    step = _gib_rows(T, P)

    def pieces():
        return (rows_of(r0, min(T, r0 + step)) for r0 in range(0, T, step))
    state = images = None
    for r0, fr in zip(range(0, T, step), pieces()):
        images, state = ops.summary_images(fr, sz, neighbours='face', state=state, first=r0 == 0, finish=r0 + step >= T)
    if isinstance(scale, str):
        if scale != 'noise':
            raise ValueError(f"denoise_movie: scale must be 'noise', None or an (X, Y, Z) image, got {scale!r}")
        scale = ops.noise_image(pieces, sz)
    return ops.lowrank_denoise(rows_of, sz, images["mean"], scale, T=T, **kw)


def _gib_rows(n, P):
    """How many of ``n`` rows of ``P`` fp32 values go through at a time: what 1 GiB holds, at least one."""
    return max(1, min(n, (1 << 30) // (4 * P)))


def lists_verdict(mode, K, boxfrac=None, nslot=None, has_nbr=None):
    """The one rule for "the neuron-list kernel forms apply", on plain values: None when they do, else the first reason they
    do not -- 'mode' (the kernel choice is neither 'auto' nor 'lists'), 'K', 'slots' (the pattern of G has too many), 'boxes'
    (a voxel lies in too many footprint boxes on average; 'lists' forces past this one), 'nbr' (no column lists for K4).
    ``boxfrac`` / ``nslot`` / ``has_nbr`` describe a layout (``ops.pack_footprints_lists``); one that is None is not tested:
    a caller passes what its kernels need, and nothing before the layout exists (it is built only for a K that passes)."""
    if mode not in ('auto', 'lists'):
        return 'mode'
    if K > LISTS_MAX_K:
        return 'K'
    if nslot is not None and nslot > ops.LISTS_MAX_SLOTS:
        return 'slots'
    # the list kernels pay per (voxel, listed neuron) and per listed pair: they win while a voxel lies in few boxes
    if mode == 'auto' and boxfrac is not None and not boxfrac < LISTS_BOXFRAC_LIMIT:
        return 'boxes'
    if has_nbr is not None and not has_nbr:
        return 'nbr'
    return None


def _pairs(n):
    """(i, j), i < j < n, in the order every by-pairs-of-groups path walks them."""
    return [(i, j) for i in range(n) for j in range(i + 1, n)]


def _dense_unions(K, group=56):   # K3 holds 127 neurons per launch
    groups = [list(range(s0, min(K, s0 + group))) for s0 in range(0, K, group)]
    return [groups[i] + groups[j] for i, j in _pairs(len(groups))]


def _gram_by_pairs(G, r, unions, launch):
    """``launch(u) -> (cols, G_u, r_u)`` on the union ``u`` of every PAIR of neuron groups, scattered into G (B,K,K) and
    r (B,K) at the neurons ``cols``.  A diagonal block is recomputed by every pair its group belongs to and the last one
    stays: the order of ``unions`` decides the bits."""
    for u in unions:
        cols, Gp, rp = launch(u)
        G[:, cols[:, None], cols[None, :]] = Gp
        r[:, cols] = rp


class _WarpRecon(torch.autograd.Function):
    """A_tC = trilinear warp of the reconstruction image S = A.C_t; differentiable w.r.t. beta."""

    @staticmethod
    def forward(ctx, beta, fp, times, C):
        times_t = torch.as_tensor(list(times), dtype=torch.int32, device=beta.device)
        Csel = C.to(device=beta.device, dtype=torch.float32).contiguous()
        S = fp.recon_image(Csel, times_t)
        out = ops.warp_recon_grad(S, None, None, None, fp.sz_list, beta.detach(), times_t, grad=None,
                                  gout=torch.zeros((len(times_t), fp.P), dtype=torch.float32, device=beta.device),
                                  want_recon=True, want_loss=False, want_reg=True)
        ctx.fp, ctx.S, ctx.times_t = fp, S, times_t
        ctx.save_for_backward(beta)
        ctx.mark_non_differentiable(out["reg"])
        return out["recon"].view(len(times_t), *fp.sz_list), out["reg"]

    @staticmethod
    def backward(ctx, g_recon, _g_reg):
        (beta,) = ctx.saved_tensors
        grad = torch.zeros_like(beta)
        gout = g_recon.contiguous().view(len(ctx.times_t), ctx.fp.P).float()
        ops.warp_recon_grad(ctx.S, None, None, None, ctx.fp.sz_list, beta.detach(), ctx.times_t, grad=grad, gout=gout,
                            want_recon=False, want_loss=False, want_reg=False)
        return grad, None, None, None


class ExponentialFP(nn.Module):
    """Gaussian footprints ``A`` deformed per frame by a quadratic map with coefficients ``beta``.

    Mirrors reference ``Demix/dNMF.py:18-122``: same constructor, same attributes (``beta`` leaf
    (10,3,T) with requires_grad, ``A`` (X,Y,Z,K), ``sigma``, ``pos``, ``sz``, ``flow_id``,
    ``transformed``), same ``forward(times, C) -> (A_tC, A_t, grid, reg)``.
    """

    def __init__(self, sz, K, T, positions=None, shape_std=3):
        super().__init__()
        ops._lib.load()  # fail here, loudly, if the HIP library is not built
        sz_t = torch.as_tensor(sz)
        self.sz_list = _sz_list(sz_t)
        X, Y, Z = self.sz_list
        self.K, self.T, self.P = int(K), int(T), X * Y * Z

        # voxel lattice and its quadratic basis (reference :22-23); kept for attribute compatibility --
        # the kernels regenerate both from the voxel index
        gx, gy, gz = torch.meshgrid(torch.arange(X), torch.arange(Y), torch.arange(Z), indexing='ij')
        flow_id = torch.stack((gx, gy, gz), 3).float().to(device)
        self.flow_id = flow_id
        self.transformed = ExponentialFP.quadratic_basis(flow_id)

        beta = torch.cat((torch.zeros(1, 3), torch.eye(3), torch.zeros(6, 3)), 0)[:, :, None].repeat(1, 1, T)
        self.beta = beta.to(device).contiguous()
        self.beta.requires_grad = True

        self.sigma = (torch.ones(K) * shape_std).to(device)
        if positions is None:
            self.pos = (1 + torch.rand(K, 3) * sz_t[None, :]).to(device)
        else:
            self.pos = positions.to(device)
        self.sz = sz_t.to(device)

        # A[x,y,z,k] = exp(-sum_d (coord_d - pos[k,d])^2 / sigma_k^2), neuron by neuron to bound the
        # temporary (the reference builds an (X,Y,Z,3,K) tensor at once, :39-40)
        A = torch.empty((X, Y, Z, K), dtype=torch.float32, device=device)
        for k in range(K):
            A[..., k] = torch.exp((-(flow_id - self.pos[k][None, None, None, :].float()) ** 2
                                   / self.sigma[k] ** 2).sum(3))
        self.A = A
        self.invalidate_layouts()
        self.use_lists = True   # reconstruction image from neuron lists when the footprints are compact
        self.last_registered_bad = None   # registered_video('linear'): int64[1] CUDA, lattice points without a solution

    def invalidate_layouts(self):
        """Forget every packed copy of ``A``.  The packed copies are keyed on ``(A.data_ptr(), A._version)``, which a
        kernel that writes ``A`` through its raw pointer (K6) does not change: such callers say so here.  A NEW dict, so
        that a shallow copy of the model (MultiChannelDNMF's channels) that calls this has a cache of its own."""
        self._layouts = {}   # name -> (key, packed copy)

    def _layout(self, name, extra, make):
        """The packed copy ``name`` of ``A``: the object of the last call while ``A`` and ``extra`` are the same, else ``make()``."""
        key = (self.A.data_ptr(), self.A._version) + extra
        hit = self._layouts.get(name)
        if hit is None or hit[0] != key:
            hit = self._layouts[name] = (key, make())
        return hit[1]

    @staticmethod
    def quadratic_basis(P):
        """[1, x, y, z, x^2, y^2, z^2, xy, xz, yz] (reference :46-51)."""
        x, y, z = P[..., 0:1], P[..., 1:2], P[..., 2:3]
        return torch.cat((x * 0 + 1, P, P * P, x * y, x * z, y * z), -1)

    def packed_footprints(self):
        """(P,Kp) zero-padded copy of ``A`` for the MFMA kernels; rebuilt when ``A`` is replaced or edited."""
        return self._layout("packed", (), lambda: ops.pack_footprints(self.A.contiguous()))

    def packed_columns(self, cols):
        """Packed copy of the footprints of the neurons ``cols`` only (K > 127 is handled by column groups: the MFMA
        kernels hold at most 8 blocks of 16 channels in registers)."""
        sub = self.A.reshape(self.P, self.K)[:, torch.as_tensor(cols, device=self.A.device)].contiguous()
        return ops.pack_footprints(sub)

    def recon_image(self, C, times, out=None, zero_state=None):
        """S[b] = A . C[:, times[b]] as (B, >= ops.halo_voxels(sz)) rows in the halo layout K2 gathers from: from the
        neuron lists when the footprints are compact (``use_lists``), else ``dnmf_recon_image`` (fp32 MFMA), by groups
        of 112 neurons when K > 127."""
        ly = self.lists_layout() if self.use_lists else None
        if ly is not None:
            # zero_state: a one-entry list the owner of a persistent ``out`` keeps -- the layout whose empty tiles are
            # known to hold zeros in these rows (written by a call without skipping); None after any other writer
            skip = zero_state is not None and zero_state[0] is ly
            res = ops.recon_image_lists(ly, self.K, self.sz_list, C, times, out=out, skip_empty=skip)
            if zero_state is not None:
                zero_state[0] = ly
            return res
        if zero_state is not None:
            zero_state[0] = None
        if self.K <= 127:
            return ops.recon_image(self.packed_footprints(), self.K, self.sz_list, C, times, out=out)
        for n, s0 in enumerate(range(0, self.K, 112)):
            cols = list(range(s0, min(self.K, s0 + 112)))
            part = ops.recon_image(self.packed_columns(cols), len(cols), self.sz_list, C[cols].contiguous(), times,
                                   out=out if n == 0 else None)
            if n == 0:
                out = part
            else:
                out[:part.shape[0], :part.shape[1]] += part
        return out

    def _zorder(self):
        """Neuron indices sorted along a Z-order curve of the footprint centroids (x,y), int32 on the GPU."""
        A2 = self.A.reshape(self.P, self.K)
        mass = A2.sum(0).clamp_min(1e-30)
        cen = (self.flow_id.reshape(self.P, 3).T @ A2) / mass            # (3,K) centroids
        q = (cen[:2] / torch.tensor(self.sz_list[:2], device=cen.device)[:, None]).clamp(0, 1 - 1e-6)
        q = (q * 1024).long().cpu().numpy()
        code = np.zeros(self.K, dtype=np.int64)
        for bit in range(10):                                           # interleave the bits of x and y
            code |= ((q[0] >> bit) & 1) << (2 * bit + 1) | ((q[1] >> bit) & 1) << (2 * bit)
        return torch.from_numpy(np.argsort(code, kind="stable").astype(np.int32)).to(device)

    @staticmethod
    def _sparse_layout(A2, order):
        Aps, mask = ops.pack_footprints_sparse(A2, order)
        nb = Aps.shape[1] // 16
        bits = (mask[:, None] >> torch.arange(nb, device=mask.device, dtype=torch.uint8)[None, :]) & 1
        return {"Aps": Aps, "order": order, "row_mask": mask, "occupancy": float(bits.float().mean())}

    def packed_sparse(self):
        """Layout for the zero-skipping Gram kernel K3s: neurons ordered along a Z-order curve of their footprint
        centroids, ``Aps`` (P,Ks) in that order, one block-occupancy byte per footprint row, and the mean
        fraction of 16-neuron blocks that are non-zero per row (``occupancy``).  None if K > 128."""
        if self.K > 128:
            return None
        return self._layout("sparse", (), lambda: self._sparse_layout(self.A.contiguous(), self._zorder()))

    # Footprint values below ``footprint_floor`` are left out of the neuron lists (K3n, the list reconstruction): 0.0 -- the
    # default -- keeps every non-zero value.  The footprint update (K5 / K6, spatial_step) is not affected: it takes its tile
    # lists and values from the layout of every non-zero value, packed_lists(floor=0).  A Gaussian footprint exp(-d^2 / 9)
    # is a non-zero fp32 number out to 30 voxels (1e-45), so its box is 61 x 61; the values beyond ~15 voxels (1e-10) enter
    # sums of order 1-10 and cannot change an fp32 result except through the ORDER of the summation (measured: the Gram
    # data and the traces move by 4e-7 relative, as they do between K3n's own launch forms).  An extension: the reference
    # has no such knob.  bench.py reports it as ``extras.footprint_floor``; the headline runs with 0.0.
    footprint_floor = 0.0

    def packed_lists(self, floor=None):
        """Layout of the neuron-list Gram kernel K3n (``ops.pack_footprints_lists``) of the values >= ``floor`` (None:
        ``footprint_floor``), rebuilt when ``A`` changes.  With ``footprint_floor == 0`` every floor of 0 is one layout."""
        floor = float(self.footprint_floor if floor is None else floor)

        def make():
            A = self.A.contiguous()
            if floor > 0:
                A = torch.where(A < floor, torch.zeros((), dtype=A.dtype, device=A.device), A)
            return ops.pack_footprints_lists(A, self.sz_list)

        # two slots: the model's own floor and one other (every non-zero value while footprint_floor > 0, the footprint update's)
        return self._layout("lists" if floor == float(self.footprint_floor) else "lists_exact", (floor,), make)

    def _lists_verdict(self, mode='auto', floor=None, slots=False, nbr=False):
        """``(packed_lists(floor), lists_verdict on it)``; ``slots`` / ``nbr``: the caller also needs the slot tables of G /
        the column lists of K4.  No layout is built when ``mode`` or K rule the lists out."""
        why = lists_verdict(mode, self.K)
        if why is not None:
            return None, why
        ly = self.packed_lists(floor)
        return ly, lists_verdict(mode, self.K, ly["boxfrac"], ly["nslot"] if slots else None,
                                 (ly["nbr"] is not None) if nbr else None)

    def lists_layout(self, forced=False, floor=None):
        """``packed_lists(floor)`` when the list kernel forms apply (``lists_verdict``; ``forced``: whatever the boxes), else None."""
        ly, why = self._lists_verdict('lists' if forced else 'auto', floor)
        return ly if why is None else None

    def packed_sparse_pairs(self, group=64):
        """K > 128: the neurons, in Z-order, are cut into groups of ``group`` and every pair of groups gets its own
        K3s layout (a mask byte holds 8 blocks of 16).  Returns ``[(cols (n,) long, layout), ...]``; ``cols`` are
        the original neuron indices of the pair, in the column order of ``layout["Aps"]`` before its own sort."""
        def make():
            z = self._zorder().long()
            groups = [z[s0:s0 + group] for s0 in range(0, self.K, group)]
            A2 = self.A.reshape(self.P, self.K)
            pairs = []
            for i, j in _pairs(len(groups)):
                cols = torch.cat([groups[i], groups[j]])
                sub = A2[:, cols].contiguous()
                ident = torch.arange(cols.numel(), dtype=torch.int32, device=device)  # already Z-ordered
                pairs.append((cols, self._sparse_layout(sub, ident)))
            return pairs

        return self._layout("sparse_pairs", (group,), make)

    def forward(self, times, C):
        """Returns ``(A_tC (B,X,Y,Z), A_t (B,K,X,Y,Z), grid (X,Y,Z,3,B), reg (B))`` for the frames ``times``."""
        times = [int(t) for t in (times.tolist() if hasattr(times, 'tolist') else times)]
        A_tC, reg = _WarpRecon.apply(self.beta, self, times, C)
        A_t, grid = ops.warp_gather(self.A.contiguous(), self.beta.detach(), times)
        return A_tC, A_t, grid, reg

    def beta_from_positions(self, P_T, ref=None, order='quadratic', ridge=0.0):
        """The warp that tracks imply: per frame t the least-squares ``beta_t`` with ``q_t(P_T[k,:,t]) = ref[k]`` (K11,
        ``ops.fit_quadratic_warp``).  ``P_T`` (K,3,T) positions of the neurons in every frame, voxel indices (what
        ``MotionCorrect.apply_shifts_points`` and the simulator produce; numpy or torch; NaN = not tracked in that frame),
        ``ref`` (K,3) the footprint centres (default ``self.pos``), ``order`` 'translation' / 'affine' / 'quadratic',
        ``ridge`` >= 0 pulls the fit to the identity.  Returns ``(beta (10,3,T) fp32 CUDA, ok (T) bool CUDA)``; a frame
        whose system is singular has the identity and ok False.  Nothing of the model is changed."""
        P = P_T if isinstance(P_T, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(P_T))
        if P.dtype not in (torch.float32, torch.float64):
            P = P.double()
        P = P.to(device)
        if P.dim() != 3 or P.shape[0] != self.K or P.shape[1] != 3:
            raise ValueError(f"beta_from_positions: positions must be ({self.K}, 3, T), got {tuple(P.shape)}")
        return ops.fit_quadratic_warp(P, self.pos if ref is None else ref, self.sz_list, order=order, ridge=ridge)

    def positions(self, points=None, times=None, start=None, tol=1e-6):
        """Where the model sees ``points`` (K,3) (default ``self.pos``, the footprint centres) in the frames ``times``
        (default all): the ``x*`` with ``q_t(x*) = points[k]`` under the current ``beta`` (K12, ``ops.invert_quadratic_warp``:
        Newton's method in float64 from ``start`` (K,3,B), default the points themselves).  Returns (K,3,B) float64 numpy in
        the layout of ``dataset.positions``; NaN where the warp has no solution Newton finds."""
        pts = self.pos if points is None else points
        if times is not None:
            times = [int(t) for t in (times.tolist() if hasattr(times, 'tolist') else times)]
        return ops.invert_quadratic_warp(self.beta.detach(), pts, times=times, start=start, tol=tol).cpu().numpy()

    @staticmethod
    def log_det_jac(B, P):
        """log|det J| of the quadratic map at ``P`` (reference :107-122, with its 8/9 row convention)."""
        x, y, z = P[0], P[1], P[2]
        # column c of the Jacobian as the reference writes it: rows 8 / 9 of beta act as the yz / xz terms
        col = [(B[1, c] + 2 * B[4, c] * x + B[7, c] * y + B[9, c] * z,
                B[2, c] + 2 * B[5, c] * y + B[7, c] * x + B[8, c] * z,
                B[3, c] + 2 * B[6, c] * z + B[8, c] * y + B[9, c] * x) for c in range(3)]
        (a, b, c), (d, e, f), (g, h, i) = col
        return torch.log(abs(a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)))

    @staticmethod
    def spatial_pushforward(dl, batch_size, sz, device, model):
        """Reference :69-93: ``A_t`` (X,Y,Z,K,T), the registered video ``Y_i`` and the raw video ``Y`` (X,Y,Z,T)
        as float64 numpy for every frame the loader yields (K1 + K7)."""
        X, Y_, Z = _sz_list(sz)
        A_list, Y_list, Yi_list = [], [], []
        for data in dl:
            times = data[1].tolist()
            beta = model.fp.beta.detach()
            A_t, _ = ops.warp_gather(model.fp.A.contiguous(), beta, times, want_grid=False)
            A_list.append(A_t.permute(2, 3, 4, 1, 0).double().cpu().numpy())
            Y_list.append(data[0].permute(1, 2, 3, 0).double().cpu().numpy())
            fr = data[0].to(device, torch.float32).reshape(len(times), -1).contiguous()
            Yi = ops.image_iwarp(fr, None, (X, Y_, Z), beta, times)
            Yi_list.append(Yi.view(len(times), X, Y_, Z).permute(1, 2, 3, 0).double().cpu().numpy())
        return np.concatenate(A_list, 4), np.concatenate(Yi_list, 3), np.concatenate(Y_list, 3)

    def registered_video(self, frames, times=None, interpolation='linear', fill=None, nchan=1):
        """The motion-corrected movie under the current ``beta``: frame b registered to the footprint volume with the warp of
        frame ``times[b]`` (None: b).  CUDA rows (B, nchan*P) in give CUDA rows (B, nchan*P) out (``nchan`` channels of a row
        share the warp); numpy or CPU-torch ``(X, Y, Z, B)`` in gives float64 numpy ``(X, Y, Z, B)`` out, the layout
        ``update_footprints`` returns ``Y_i`` in.

        ``interpolation='linear'`` (K17, ``ops.warp_pullback``): for every lattice point u the x with q_t(x) = u, and the frame
        sampled trilinearly there with zero padding -- the model's own forward read backwards, smooth in the warp.  It works in
        true voxel coordinates and does NOT carry the ``sz``-for-``sz - 1`` un-normalisation quirk that ``spatial_pushforward``
        keeps from the reference: an extension, not a parity path.  ``fill``: None = zero padding and 0 where the warp has no
        solution Newton finds; a float (NaN, say) marks every point that comes from outside the frame, and those.
        ``self.last_registered_bad`` then holds the number of lattice points without a solution (an int64 CUDA tensor).
        ``interpolation='nearest'``: the reference's nearest-neighbour registration (K7, ``ops.image_iwarp``), which has no
        ``fill``."""
        if interpolation not in ('linear', 'nearest'):
            raise ValueError(f"registered_video: interpolation must be 'linear' or 'nearest', got {interpolation!r}")
        if interpolation == 'nearest' and fill is not None:
            raise ValueError("registered_video: fill applies to interpolation='linear' only")
        X, Y, Z = self.sz_list
        on_gpu = isinstance(frames, torch.Tensor) and frames.is_cuda
        if on_gpu:
            if frames.dim() != 2:
                raise ValueError(f"registered_video: CUDA frames are rows (B, nchan*P), got {tuple(frames.shape)}")
            rows = frames
        else:
            v = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
            if v.dim() != 4 or list(v.shape[:3]) != [X, Y, Z] or nchan != 1:
                raise ValueError(f"registered_video: host frames are ({X}, {Y}, {Z}, B) with one channel, got {tuple(v.shape)}")
            rows = v.to(device, torch.float32).permute(3, 0, 1, 2).reshape(v.shape[3], -1).contiguous()
        if times is None:
            times = torch.arange(rows.shape[0], dtype=torch.int32, device=device)
        beta = self.beta.detach()
        if interpolation == 'linear':
            self.last_registered_bad = torch.zeros(1, dtype=torch.int64, device=device)
            out = ops.warp_pullback(rows, None, self.sz_list, beta, times, nchan=nchan, fill=fill, count=self.last_registered_bad)
        else:
            self.last_registered_bad = None
            out = ops.image_iwarp(rows, None, self.sz_list, beta, times, nchan=nchan)
        if on_gpu:
            return out
        return out.view(-1, X, Y, Z).permute(1, 2, 3, 0).double().cpu().numpy()

    @staticmethod
    def image_iwarp(im, flow, grid):
        """Reference :95-103: the value of ``im`` at the flow point nearest to each query of ``grid`` (scipy's
        NearestNDInterpolator), reshaped to ``im.shape``.  ``im`` (X,Y,Z) values, ``flow`` (X,Y,Z,3) the position of every
        voxel of ``im`` (same order), ``grid`` (..., 3) query points, integer or float, one per voxel of ``im``.

        K10 (``ops.nearest_points``): float64 distances on the flow as stored, exact; exact ties go to the lowest voxel index
        (cKDTree leaves that choice unspecified).  numpy or CPU-torch ``im`` gives a numpy array of ``im``'s dtype, as the
        reference does; a CUDA ``im`` gives a CUDA tensor (an extension of the reference).  Raises ValueError when the
        number of flow points or queries is not ``im``'s size, or when a coordinate is not finite."""
        on_gpu = isinstance(im, torch.Tensor) and im.is_cuda
        vals = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im))
        shape = tuple(vals.shape)
        n = vals.numel()
        fl = flow if isinstance(flow, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(flow))
        if fl.dtype not in (torch.float32, torch.float64):
            fl = fl.double()
        pts = fl.to(device).reshape(-1, 3)
        q = torch.as_tensor(np.asarray(grid) if not isinstance(grid, torch.Tensor) else grid)
        q = q.to(device=device, dtype=torch.float64).reshape(-1, 3)
        if pts.shape[0] != n or q.shape[0] != n:
            raise ValueError(f"image_iwarp: {pts.shape[0]} flow points and {q.shape[0]} queries for an image of {n} values")
        if vals.dtype == torch.float32:
            _, out = ops.nearest_points(pts[None], q, values=vals.to(device).reshape(1, n))
            out = out.reshape(shape)
        else:
            idx = ops.nearest_points(pts[None], q)
            flat = vals.reshape(-1)
            out = torch.take(flat, idx.reshape(-1).to(device=flat.device, dtype=torch.int64)).reshape(shape)
        return out if on_gpu else out.cpu().numpy()

    @staticmethod
    def detect_positions(image, K, shape_std=3, **kw):
        """Where the neurons are in a template volume ``image`` (X,Y,Z) -- a frame, a mean image, ``MotionCorrect``'s
        template: ``(positions (K,3), amplitudes (K,))`` of up to K blobs exp(-|x - p|^2 / shape_std^2), brightest first, by
        K14 (``ops.detect_neurons``, whose ``min_distance``, ``threshold`` and ``background`` pass through ``kw``).  Rows
        beyond the number found are NaN, the "not tracked" of ``init_motion``.  numpy or CPU-torch in, numpy out; a CUDA
        ``image`` gives CUDA tensors.  The reference has no counterpart: its real data comes with annotated positions."""
        on_gpu = isinstance(image, torch.Tensor) and image.is_cuda
        img = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
        if img.dim() != 3:
            raise ValueError(f"detect_positions: image must be (X,Y,Z), got {tuple(img.shape)}")
        img = img.to(device, torch.float32).contiguous()
        pos, amp, _ = ops.detect_neurons(img, img.shape, K, shape_std=shape_std, **kw)
        return (pos, amp) if on_gpu else (pos.cpu().numpy(), amp.cpu().numpy())

    @staticmethod
    def _video_rows(video, name):
        """(rows (T, ld) fp32 CUDA, [X, Y, Z], rows came from the GPU) of a video given as (T, X, Y, Z) values (numpy / torch), as
        resident rows with their volume ``(rows (T, P), sz)``, or as a ``ResidentLoader``."""
        if hasattr(video, "frames_2d"):
            return video.frames_2d(), _sz_list(video.sz), True
        if isinstance(video, (tuple, list)) and len(video) == 2 and getattr(video[0], "ndim", 0) == 2:
            rows, sz = video
            on_gpu = isinstance(rows, torch.Tensor) and rows.is_cuda
            rows = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rows))
            rows = rows.to(device, torch.float32)
            return (rows if rows.stride(1) == 1 else rows.contiguous()), _sz_list(sz), on_gpu
        on_gpu = isinstance(video, torch.Tensor) and video.is_cuda
        v = video if isinstance(video, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(video))
        if v.dim() != 4:
            raise ValueError(f"{name}: a video is (T, X, Y, Z), (rows (T, P), sz) or a ResidentLoader, got {tuple(v.shape)}")
        return v.to(device, torch.float32).reshape(v.shape[0], -1).contiguous(), [int(n) for n in v.shape[1:]], on_gpu

    @staticmethod
    def summary_images(video, neighbours='full'):
        """The summary images of ``video`` -- (T, X, Y, Z) values, ``(rows (T, P), sz)`` or a ``ResidentLoader``, as
        ``track_positions`` takes it: a dict ``mean / std / max / corr`` of (X, Y, Z) float64 images by K18
        (``ops.summary_images``): per voxel the mean, the population std and the max over time, and the local correlation
        image, the mean Pearson correlation of the voxel with its ``neighbours`` ('full': 26, 8 at Z = 1; 'face': 6 / 4).
        The max, std and correlation images show neurons that are dim on average but active, which a mean image hides: the
        usual seeds for ``detect_positions``.  A voxel without a neighbour of non-zero variance has corr = NaN; a voxel with
        a sample that is not finite is NaN in all four.  numpy or CPU-torch in, numpy out; CUDA frames give CUDA tensors."""
        rows, sz, on_gpu = ExponentialFP._video_rows(video, "summary_images")
        images, _ = ops.summary_images(rows, sz, neighbours=neighbours)
        return images if on_gpu else {k: v.cpu().numpy() for k, v in images.items()}

    @staticmethod
    def robust_images(video, percentiles=(), noise='diff'):
        """The order-statistic images of ``video`` -- (T, X, Y, Z) values, ``(rows (T, P), sz)`` or a ``ResidentLoader``, as
        ``summary_images`` takes it -- by K30 (``ops.robust_images``, exact selection, the same bits on every run): a dict of
        (X, Y, Z) float64 images ``median``, ``max``, ``mad`` (median |y - median|), ``noise`` (``'diff'``: the median absolute
        difference of adjacent frames x 1.4826 / sqrt(2), what ``deconvolve`` estimates per trace; ``'mad'``: 1.4826 mad),
        ``pnr`` = (max - median) / noise, ``n`` (int32: the finite samples of the voxel; the others are left out) and
        ``percentile`` {p: image} for every p of ``percentiles`` (8 gives an F0 image).  ``median`` is a baseline no transient
        pulls up; ``pnr`` shows a cell that is dim on average but active, however narrow, where ``max`` and ``std`` show what is
        bright and noisy; ``corr`` x ``pnr`` is the usual seed image.  pnr is NaN where noise is 0 or not finite or n < 2.
        numpy or CPU-torch in, numpy out; CUDA frames give CUDA tensors."""
        rows, sz, on_gpu = ExponentialFP._video_rows(video, "robust_images")
        images = ops.robust_images(rows, sz, percentiles, noise)
        return images if on_gpu else _images_to_numpy(images)

    @staticmethod
    def dff_movie(video, window, stride=None, percentile=8.0, mode='dff', offset=0.0, min_samples=1):
        """``video`` -- (T, X, Y, Z) values, ``(rows (T, P), sz)`` or a ``ResidentLoader``, as ``robust_images`` takes it, its rows
        in time order -- read against its own slowly moving baseline (K31, ``ops.running_quantile`` and ``ops.baseline_apply``;
        tests/dff_restatement.py): per voxel the ``percentile`` of every window of ``window`` frames, one every ``stride`` frames
        (None: a quarter of the window), exact and interpolated as ``np.nanquantile`` does, joined by straight lines between the
        window centres and held flat outside them -> ``(movie, info)``.  ``mode``: ``'dff'`` (y - F0) / (F0 + offset), ``'df'``
        y - F0, ``'dfsqrtf'`` (y - F0) / sqrt(F0 + offset), ``'baseline'`` F0 itself; NaN where the sample or the baseline is not
        finite (a window with fewer than ``min_samples`` finite samples has none) or F0 + offset <= 0.  A session that bleaches
        has no single F0: the one 8th percentile of ``robust_images`` sits at its end-of-session level.  ``info``: ``knots``
        (J, X, Y, Z) float64, ``centres``, ``n`` (J, X, Y, Z), ``starts``, ``ends``.  CUDA frames give CUDA rows (T, P) and CUDA
        ``knots`` / ``n``; numpy or CPU-torch in, numpy float32 (T, X, Y, Z) out.  Unlike CaImAn's ``detrend_df_f`` the knots are
        joined linearly (not by a cubic zoom), the windows at the two ends are clamped to the movie (not padded), and the
        percentile is interpolated (``method='linear'``), not the nearest rank."""
        if not 0.0 <= float(percentile) <= 100.0:
            raise ValueError(f"dff_movie: percentile must lie in [0, 100], got {percentile!r}")
        rows, sz, on_gpu = ExponentialFP._video_rows(video, "dff_movie")
        movie, info = ops.dff_rows(lambda r0, r1: rows[r0:r1], rows.shape[0], sz, window, stride, float(percentile) / 100.0, mode,
                                   offset, min_samples)
        if on_gpu:
            return movie, info
        info = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in info.items()}
        return movie.cpu().numpy().reshape(rows.shape[0], *sz), info

    @staticmethod
    def denoise_movie(video, patch=(16, 16, None), overlap=(8, 8, 0), rank=8, keep='auto', threshold=1.0, iters=4, scale='noise'):
        """A registered (or nearly static) ``video`` denoised by local low-rank approximation (K34, ``ops.lowrank_denoise``;
        tests/denoise_restatement.py): the volume is covered by overlapping patches of ``patch`` voxels (``None`` in z: min(Z, 4);
        at most 1024 voxels), in each the ``rank`` <= 8 leading singular pairs of (y - mean) / scale are found by ``iters`` steps of
        subspace iteration, those above ``threshold`` x the noise edge sqrt n + sqrt T are kept (``keep='auto'``; a number keeps
        that many), and the patches are blended by tent weights -> ``(movie, info)``.  ``scale``: ``'noise'`` (K30's noise image,
        which makes the noise of every voxel unit), ``None`` (ones) or an (X, Y, Z) image.  Inside a patch a registered movie is a
        handful of components plus independent noise; in frame coordinates a moving animal is not, so register first
        (``DeformableNMF.denoise_movie(registered=)``).  ``info``: ``plan``, ``kept`` (NP,), ``lam`` (NP, R), ``ok``, ``explained``
        and the factors ``U`` (NP, n, R), ``Q`` (NP, T, R) -- a compressed form of the movie.  A patch with a sample that is not
        finite, or a voxel of zero noise, is left out (``ok`` = 0); a voxel no other patch covers comes back as it is.
        ``video``: (X, Y, Z, T) values (numpy or torch) give a float32 numpy (X, Y, Z, T) movie and numpy ``info``; CUDA rows with
        their volume ``(rows (T, P), sz)`` or a ``ResidentLoader`` give CUDA rows (T, P) and CUDA ``info``, as ``dff_movie``."""
        if hasattr(video, "frames_2d") or (isinstance(video, (tuple, list)) and len(video) == 2):
            rows, sz, on_gpu = ExponentialFP._video_rows(video, "denoise_movie")
        else:
            v = video if isinstance(video, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(video))
            if v.dim() != 4:
                raise ValueError(f"denoise_movie: a video is (X, Y, Z, T), (rows (T, P), sz) or a ResidentLoader, got {tuple(v.shape)}")
            sz, on_gpu = [int(n) for n in v.shape[:3]], False
            rows = v.to(device, torch.float32).permute(3, 0, 1, 2).reshape(v.shape[3], -1).contiguous()
        movie, info = _denoise_rows(lambda r0, r1: rows[r0:r1], rows.shape[0], sz, scale, patch=patch, overlap=overlap, rank=rank,
                                    keep=keep, threshold=threshold, iters=iters)
        if on_gpu:
            return movie, info
        info = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in info.items()}
        return movie.view(-1, *sz).permute(1, 2, 3, 0).cpu().numpy(), info

    @staticmethod
    def background(video, iters=3):
        """The rank-1 background of ``video`` as it is (K19, ``ops.background_fit``): ``(b (X, Y, Z), f (T,))`` fp32, both >= 0
        with mean(f) = 1, after ``iters`` alternations of the two exact coordinate steps of ``min |video - b f|^2`` from b = 1.
        ``video``: (T, X, Y, Z) values, ``(rows (T, P), sz)`` or a ``ResidentLoader``, as ``summary_images`` takes it.  On a
        movie that also shows neurons, b holds their time-averaged light as well: ``DeformableNMF.update_background`` fits the
        background on what the model leaves.  numpy or CPU-torch in, numpy out; CUDA frames give CUDA tensors."""
        rows, sz, on_gpu = ExponentialFP._video_rows(video, "background")
        b, f = ops.background_fit(rows, sz, iters)
        return (b, f) if on_gpu else (b.cpu().numpy(), f.cpu().numpy())

    @staticmethod
    def background_rank(video, iters=3, rank=2, inner=3):
        """The rank-R background of ``video`` as it is (K23, ``ops.background_fit_rank``), 2 <= R <= 8: R images and R time courses,
        ``(b (R, X, Y, Z), f (R, T))`` fp32, all >= 0 with mean(f_j) = 1, for a movie whose background has sources with different
        time courses (a constant offset, a decaying glow, a rising one).  ``video`` and the return types as ``background`` has
        them; ``rank=1`` is ``background(video, iters)``."""
        if rank == 1:
            return ExponentialFP.background(video, iters)
        rows, sz, on_gpu = ExponentialFP._video_rows(video, "background_rank")
        b, f = ops.background_fit_rank(rows, sz, iters, rank, inner=inner)
        return (b, f) if on_gpu else (b.cpu().numpy(), f.cpu().numpy())

    @staticmethod
    def track_positions(video, points, shape_std=3, search=(6, 6, 1), predict=None, threshold=0.0, background=None, **kw):
        """Where the neurons are in every frame of ``video`` -- (T, X, Y, Z) values, or frames that already live on the GPU as
        ``(rows (T, P), sz)`` or a ``ResidentLoader``: ``(P_T (K,3,T) float64, amplitudes (K,T))`` by K15
        (``ops.track_neurons``): per neuron and frame the sub-voxel peak of the frame's matched-filter score (K14's, with
        exp(-|x - p|^2 / shape_std^2)) within ``search`` voxels per axis of the rounded prediction, and its least-squares
        amplitude.  ``points`` (K,3): the centres in one frame, annotated or detected (``detect_positions``); ``predict``
        (K,3,T) or (K,3): where to look in every frame (None: at ``points``) -- it carries any prior, frame t is not chained
        on frame t - 1.  NaN = not found (the "not tracked" of ``init_motion``): the prediction is not finite, the window
        misses the volume, or the peak is not above ``threshold``.  ``background``: None (0), a number or T values taken off
        the frames.  The searches are independent and neighbouring neurons are not removed from the score: a neuron within
        about 2 shape_std of a brighter one can be captured by it, and ``search`` is the guard against that -- unless the
        one further keyword ``exclude=R`` (default 0: the call as described) is R >= 1: K15 then runs once for the peaks, each
        frame's neurons are ordered by them (descending, stable, NaN last) and K15x (``ops.track_neurons_exclusive``)
        searches them in that order, every neuron on the frame less the model footprints of those already placed, in R
        rounds -- the brighter neuron no longer hides the dimmer one.  Two neurons that K15 finds on the same voxel have
        equal peaks and keep the order of their indices.  ``follow_positions`` has no such mode.  numpy or CPU-torch in,
        numpy out; a CUDA ``video`` gives CUDA tensors.  The reference has no counterpart."""
        exclude = int(kw.pop("exclude", 0))
        if kw:
            raise TypeError(f"track_positions: unexpected keyword arguments {sorted(kw)}")
        if exclude < 0:
            raise ValueError(f"track_positions: exclude={exclude} must not be negative")
        rows, sz, on_gpu = ExponentialFP._video_rows(video, "track_positions")
        pred = points if predict is None else predict
        pred = pred if isinstance(pred, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pred))
        if pred.dtype not in (torch.float32, torch.float64):
            pred = pred.double()
        pred = pred.to(device)
        K = len(points)
        if pred.dim() not in (2, 3) or pred.shape[0] != K or pred.shape[1] != 3:
            raise ValueError(f"track_positions: predict must be ({K}, 3, T) or ({K}, 3), got {tuple(pred.shape)}")
        pos, amp, peaks = ops.track_neurons(rows, sz, pred, shape_std=shape_std, search=search, threshold=threshold, background=background)
        if exclude:
            order = torch.argsort(torch.nan_to_num(peaks, nan=float("-inf")), dim=0, descending=True, stable=True).int()
            pos, amp, _, _ = ops.track_neurons_exclusive(rows, sz, pred, order, shape_std=shape_std, search=search, rounds=exclude,
                                                         threshold=threshold, background=background)
        return (pos, amp) if on_gpu else (pos.cpu().numpy(), amp.cpu().numpy())

    @staticmethod
    def follow_positions(video, points, shape_std=3, search=(3, 3, 1), anchor=0, momentum=0.0, max_gap=5, threshold=0.0, background=None):
        """The neurons followed through ``video`` (what ``track_positions`` takes) from their centres ``points`` (K,3) in the
        frame ``anchor``, forwards and backwards, by K15c (``ops.follow_neurons``): ``(P_T (K,3,T) float64, amplitudes (K,T),
        info)``, ``info`` a dict ``predicted (K,3,T), peaks (K,T), lost_at (K,2)``.  Unlike ``track_positions`` frame t is
        chained on frame t -+ 1: it is searched within ``search`` voxels of the last position found plus ``momentum`` times
        the last step, so a neuron that moves little per frame and far in total is followed with a small window -- the
        guard against capture by a brighter neighbour -- and ``momentum=1`` follows one that moves further per frame than
        the window is wide.  NaN = not found; after more than ``max_gap`` such frames in a row the chain is lost from
        ``lost_at[k]`` (forward, backward; -1: never) on.  ``P_T`` feeds ``init_motion``, ``positions`` and ``roi_signals``
        as tracks from anywhere.  The T steps of a chain are sequential and there is still no exclusion between neurons: a
        neuron within about 2 shape_std of a brighter one can be captured by it.  numpy or CPU-torch in, numpy out; a CUDA
        ``video`` gives CUDA tensors.  The reference has no counterpart."""
        rows, sz, on_gpu = ExponentialFP._video_rows(video, "follow_positions")
        pts = points if isinstance(points, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(points))
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"follow_positions: points must be (K, 3), got {tuple(pts.shape)}")
        out = ops.follow_neurons(rows, sz, pts.double().to(device), shape_std=shape_std, search=search, anchor=anchor, momentum=momentum,
                                 max_gap=max_gap, threshold=threshold, background=background)
        if not on_gpu:
            out = {k: v.cpu().numpy() for k, v in out.items()}
        return out["positions"], out["amplitudes"], dict(predicted=out["predicted"], peaks=out["peaks"], lost_at=out["lost_at"])


class DeformableNMF:
    """Reference ``Demix/dNMF.py:124-194``: owns the spatial model ``fp`` and the traces ``C`` (K,T)."""

    # footprint width the constructor builds ``fp`` with: the reference's 3; from_image sets its own on the instance first
    _shape_std = 3
    # the volume-preserving prior of update_motion(solver='gn') is off unless an instance sets a weight (see __init__)
    motion_jacobian = 0.0

    def __init__(self, sz, K, T, positions=None):
        self.SpatialModel = ExponentialFP
        self.fp = self.SpatialModel(sz=sz, K=K, T=T, positions=positions, shape_std=self._shape_std)
        self.C = torch.rand((K, T)).to(device)
        self.A = torch.rand((K, _sz_list(sz)[0], _sz_list(sz)[1])).to(device)  # unused in the reference too (:131)
        self.verbose = True
        self.D = None if positions is None else self._distance_prior(positions).reshape(*_sz_list(sz), K)
        self._ws_k2 = None
        self._ws_k3 = None
        self._S_bufs = None
        self._S_zero = None
        self._gram_nbr = None   # (K,NN) columns of the last Gram matrices that can be non-zero, when K3n made them
        # after update_footprints(solver='hals'): per frame of that call the largest projected-gradient entry of the
        # trace problem on the solver's float64 state, before self.C is rounded to float32 (float64 CPU tensor; zero at the
        # NNLS solution); None after a solver='mu' call
        self.last_temporal_kkt = None
        # after update_footprints(solver='ar1'): g, penalty, baseline, s, colour, n_colours, n_pools, n_weightless, F of that
        # call (see there); None after another solver
        self.last_temporal_ar = None
        self.last_spatial_kkt = None  # (K,) float64 after a spatial_step(solver='hals'), None after a 'mu' step
        # update_motion evaluates a whole epoch per launch when the caller's optimiser is a plain
        # torch.optim.Adam on [fp.beta] and the loader is a ResidentLoader (same result, see _motion_epoch)
        self.fused_motion = True
        # Gram kernel: 'dense' = K3 (every product evaluated), 'sparse' = K3s (16-neuron blocks that are exactly zero
        # skipped), 'lists' = K3n (only the neurons whose non-zero box a tile of voxels can reach; same sums),
        # 'auto' = K3n while a voxel lies in few boxes, else K3s when on average fewer than half of the 16-neuron
        # blocks of a footprint row are non-zero, else K3, 'bf16' = K3b (every product, operands rounded to bf16: reduced precision the
        # reference does not have, never chosen by 'auto')
        self.gram_kernel = 'auto'
        # footprint update (spatial_step): 'lists' = K5 / K6 on (tile, listed neuron) pairs only, 'dense' = the MFMA K5 on all
        # P x K entries, 'auto' = lists while the footprints are compact
        self.spatial_kernel = 'auto'
        self._sl = None
        self._ws_k5 = None
        # torch.distributed group when this object holds one contiguous T-shard per rank (rank order = frame order);
        # used where the path has a real exchange: the neighbour term of update_temporal and spatial_step
        self.group = None
        self._comm = None  # ops.Communicator over self.group, built by spatial_step when collective == "c1"
        # the one collective of the path (spatial_step): 'torch' = torch.distributed.all_reduce on self.group (RCCL under the
        # "nccl" backend); 'c1' = dnmf_allreduce_sum_f32 on the library's own communicator.  C1 has only ever run with one
        # rank (one GPU per test box), so it is not the default
        self.collective = "torch"
        self._spatial_buf = None   # A1 (P,K) and C_s (K,K) of spatial_step, one buffer = one all-reduce
        self._ws_mg = None
        # > 0: the fused motion epoch on compact footprints makes its reconstruction images this many frames at a time
        # into one small buffer (dnmf_motion_grad_lists) instead of keeping the images of all T frames (4.5 GB at
        # 512x512x4000): same results bit for bit, same speed within 2 % from 128 frames on (the hoped-for gain from
        # images that stay in the Infinity Cache did not materialise), so it is a memory option; 0 = all frames at once
        self.motion_chunk = 0
        # weight of the temporal smoothness prior of update_motion(solver='gn') (K16s, see _update_motion_gn): mean squared
        # error per squared voxel of frame-to-frame change of a warp coefficient.  0 = none, every frame fitted on its own.  An
        # attribute like motion_chunk, not a parameter: update_motion keeps the parameter list it had
        self.motion_smooth = 0.0
        # which coefficients update_motion(solver='gn') fits (K16o, see _update_motion_gn): 'translation', 'affine' or
        # 'quadratic' (the default: all of them, the path as it was), 'graded' = the three in turn, or any sequence of
        # (order, iterations) stages.  An attribute for the same reason
        self.motion_order = 'quadratic'
        # weight of the volume-preserving prior of update_motion(solver='gn') (K16j, see _update_motion_gn): mean squared error
        # per squared unit of log det J of a frame's map at the corners and the centre of the volume; a map that folds there is
        # never accepted.  0 = none, the path as it was.  An attribute for the same reason
        self.motion_jacobian = 0.0
        self._stage_buf = None     # device copy of the frames a host loader served in its last pass
        # after update_motion(solver='gn'): per frame sse0, sse, accepted, rejected, lam -- and prior when smooth > 0, jac and
        # min_det when motion_jacobian > 0 -- (CUDA tensors, (T,)), and stages when motion_order is set: a list, per stage a
        # dict(order, sse0, sse); else None
        self.last_motion_gn = None
        self._reg_buf = None       # registered frames (K7 / K17) of the last update_footprints(live_spatial=True)
        self.last_registered_bad = None   # registered_video('linear'): lattice points the warp had no solution for
        self._D_dev = None         # (id(self.D), fp32 device copy of D flattened to (P,K))
        self.stream_loader = True  # stage host loaders on the GPU once per pass (see _stage_epoch)
        # after update_background: (b (X,Y,Z), f (T,)) fp32 CUDA, the rank-1 background b f_t of frame t in frame coordinates;
        # after update_background_rank with R >= 2: (b (R,X,Y,Z), f (R,T)), the background sum_j b_j f_j[t]
        self.background = None
        # after clean_traces: a, b, F0, fitted, n_outliers per neuron (CUDA tensors, (K,)) of that call
        self.last_clean = None
        # after dff_movie: knots (J,X,Y,Z) float64, centres, n, starts, ends of that call; after detrend_traces: baseline (K,T)
        self.last_dff = None
        self.last_detrend = None
        # after deconvolve: g, penalty, baseline, noise, rss, n_valid, n_pools, ok per neuron (CUDA tensors, (K,)) of that call
        self.last_deconv = None
        # after match_traces: beta (K, 2), distance (K,), ok (K,) of that call (CUDA tensors)
        self.last_match = None
        # after follow: (P_T (K,3,T), amplitudes (K,T), info) of that call
        self.last_follow = None
        # after evaluate_components: r_values, snr, frame_corr, raw, images, boxes, n_active and keep of that call
        self.last_evaluation = None
        # after merge_components: pairs, overlap, corr, groups, merged and K of that call
        self.last_merge = None
        # after clean_footprints: the eight per-neuron statistics and the boxes of that call
        self.last_footprint_clean = None
        # after add_components: centres, boxes, explained, energy, ok, kept, added and K of that call
        self.last_add = None
        # after denoise_movie: plan, kept, lam, ok, explained and the factors U, Q of that call
        self.last_denoise = None
        self._warned = set()

    @classmethod
    def from_image(cls, image, K, T, shape_std=3, **kw):
        """A model on the centres ``ExponentialFP.detect_positions(image, K, shape_std, **kw)`` finds in ``image`` (X,Y,Z): as
        many neurons as were found (at most K; ValueError when none), footprints of width ``shape_std``, the width the
        detection matched."""
        pos, _ = ExponentialFP.detect_positions(image, K, shape_std=shape_std, **kw)
        pos = torch.as_tensor(pos).to(device)
        n = int(torch.isfinite(pos).all(1).sum())     # the found rows come first
        if n == 0:
            raise ValueError(f"from_image: no neuron found in the image (K={K}, shape_std={shape_std}, {kw})")
        sz = torch.tensor([int(s) for s in image.shape])
        positions = pos[:n].float().contiguous()
        model = cls.__new__(cls)
        model._shape_std = shape_std                  # read by __init__ where it builds fp
        model.__init__(sz, n, T, positions=positions)
        return model

    # ---- static NMF updates (numpy in / numpy out like the reference) ---------------------------------
    @staticmethod
    def update_temporal(A_t, C, Y, gamma=None, solver='mu', iters=1):
        """One multiplicative update of ``C`` given explicit warped footprints (reference :139-149); ``iters`` of them, or
        with ``solver='hals'`` ``iters`` sweeps of the exact coordinate-descent solver K4h on the same Gram data.
        ``A_t`` (X,Y,Z,K,T), ``C`` (K,T), ``Y`` (X,Y,Z,T) numpy; returns float64 numpy (K,T).  The contraction runs on
        the fp32 matrix cores (K3 without a warp: every voxel's own row of ``A_t``), the update in float64 (K4); more than
        127 neurons go by pairs of neuron groups (one K3 launch holds 127)."""
        _check_solver(solver)
        A_t, C, Y = np.asarray(A_t), np.asarray(C), np.asarray(Y)
        X, Y_, Z, K, T = A_t.shape
        P = X * Y_ * Z
        dev = torch.device(device)
        A_dev = torch.from_numpy(np.ascontiguousarray(np.moveaxis(A_t, 4, 0).reshape(T, P, K))).to(dev, torch.float32)
        frames = torch.from_numpy(np.ascontiguousarray(np.moveaxis(Y, 3, 0).reshape(T, P))).to(dev, torch.float32)

        def gram(cols):
            idx = None if cols is None else torch.as_tensor(cols, device=dev)
            sub = A_dev if idx is None else A_dev[:, :, idx].contiguous()
            Apk = ops.pack_footprints(sub)                                 # (T*P, Kp)
            return (idx,) + ops.warp_gram_rhs(Apk, sub.shape[2], (X, Y_, Z), None, list(range(T)), frames,
                                              a_frame_stride=P * Apk.shape[1])[:2]

        if K <= 127:
            _, G, r = gram(None)
        else:
            # one K3 launch holds 127 neurons: groups of 56 by pairs, as DeformableNMF._gram_rhs_grouped does on the fit path
            G = torch.empty((T, K, K), dtype=torch.float32, device=dev)
            r = torch.empty((T, K), dtype=torch.float32, device=dev)
            _gram_by_pairs(G, r, _dense_unions(K), gram)
        C0 = torch.from_numpy(np.asarray(C, dtype=np.float64)).to(dev)
        if solver == 'hals':
            return _hals_temporal(G, r, C0, gamma, iters)[0].cpu().numpy()
        return _mu_temporal(G, r, C0, gamma, iters).cpu().numpy()

    @staticmethod
    def update_spatial(A, C, Y_i, D=None, gamma=None, solver='mu', sweeps=1, boxes=None):
        """One multiplicative update of un-warped footprints (reference :151-160): numpy in, float64 numpy out.
        ``A`` (..., K), ``C`` (K,T), ``Y_i`` (..., T), ``D`` None or like ``A``; the leading axes are the voxels
        (the reference's einsum strings accept two of them, any number works here).  K5 + K6, fp32 MFMA.
        ``solver='hals'`` (extension): the dense K5, then ``sweeps`` sweeps of the exact solver K6h (``ops.hals_spatial``)
        instead of the one multiplicative update; ``boxes`` (K,6) restricts neuron k to its box of the volume ``A.shape[:-1]``
        (up to three axes), None leaves every voxel free."""
        _check_solver(solver)
        if solver == 'mu' and (boxes is not None or sweeps != 1):
            raise ValueError("update_spatial: sweeps and boxes belong to solver='hals'")
        A, C, Y_i = np.asarray(A), np.asarray(C), np.asarray(Y_i)
        K, T = C.shape
        dev = torch.device(device)
        A_dev = torch.from_numpy(np.ascontiguousarray(A.reshape(-1, K))).to(dev, torch.float32)
        Y_dev = torch.from_numpy(np.ascontiguousarray(Y_i.reshape(-1, T).T)).to(dev, torch.float32)
        C_dev = torch.from_numpy(np.ascontiguousarray(C)).to(dev, torch.float32)
        D_dev = None if D is None else torch.from_numpy(np.ascontiguousarray(np.asarray(D).reshape(-1, K))).to(dev, torch.float32)
        A1, Cs = torch.empty_like(A_dev), torch.empty((K, K), dtype=torch.float32, device=dev)
        DeformableNMF._spatial_accum_dense(Y_dev, C_dev, A1, Cs, None, None)
        if solver == 'hals':
            sz = None
            if boxes is not None:
                if A.ndim > 4:
                    raise ValueError(f"update_spatial: boxes need at most three voxel axes, A is {A.shape}")
                sz = tuple(A.shape[:-1]) + (1,) * (4 - A.ndim)
            ops.hals_spatial(A_dev, A1, Cs, D_dev, gamma, sweeps=sweeps, boxes=boxes, sz=sz)
        else:
            ops.mu_spatial(A_dev, A1, Cs, D_dev, gamma)
        return A_dev.double().cpu().numpy().reshape(A.shape)

    def spatial_step(self, registered, D=None, gamma=None, frame_ids=None, times=None, solver='mu', sweeps=1, grow=0):
        """One multiplicative update of ``fp.A`` from the registered frames this process holds (the update the
        reference leaves commented out at :174, on the flattened voxel axis): K5 on the local frames, ONE all-reduce
        (sum) of the buffer that holds ``A1`` (P,K) and ``C_s`` (K,K) over ``self.group`` when the T axis is sharded,
        then K6 -- every rank ends with the same footprints.  ``registered`` (>=T_local,P) fp32 CUDA rows, frame b in
        row ``frame_ids[b]`` (None: b) with trace column ``times[b]`` (None: ``frame_ids[b]``, else b); ``D`` None or
        (X,Y,Z,K).  ``self.last_spatial_ms`` receives (K5, all-reduce, K6) HIP-event times when ``self.time_spatial``
        is set.

        ``solver='hals'`` (extension): the same K5, all-reduce and ``_scale_Cs``, then ``sweeps`` sweeps of the exact
        solver K6h in one launch -- cyclic coordinate descent on the non-negative least-squares problem of every voxel, which
        the multiplicative update only approaches, can revive a zero and takes sums of any sign.  The support of neuron k is
        the box of its non-zero values grown by ``grow`` voxels (an int or (gx, gy, gz)) and clipped to the volume; with
        ``grow != 0`` the tile lists of K5 and K6h are made from the grown boxes (the cached lists of the 'mu' path are left
        alone), and the dense form takes the same boxes, so the result does not depend on the form.
        ``self.last_spatial_kkt`` (K,) float64 then holds, per neuron, how far the float64 state was from the solution after
        the last sweep (largest projected-gradient entry); it is None after a 'mu' step."""
        _check_spatial_solver(solver, sweeps, grow, "spatial_step")
        fp = self.fp
        P, K = fp.P, fp.K
        C = self.C.to(device, torch.float32).contiguous()
        if times is None:
            times = frame_ids
        hals = solver == 'hals'
        if hals:
            boxes, sl = self._spatial_support(grow)
        else:
            sl = self._spatial_lists()
        # A1 and C_s live in one buffer so that the exchange is a single collective; with compact footprints A1 exists
        # only for (tile, listed neuron) pairs -- a few floats per voxel instead of K (3 MB instead of 105 MB at cfg 3)
        n1 = sl["total"] if sl is not None else P * K
        buf = self._spatial_buffer(n1 + K * K)
        Cs = buf[n1:].view(K, K)
        A1 = buf[:n1] if sl is not None else buf[:n1].view(P, K)
        self._spatial_numerator(registered, C, sl, A1, Cs, frame_ids, times)
        self._allreduce_spatial(buf)
        self._scale_Cs(Cs)
        A2 = fp.A.reshape(P, K).contiguous()
        Dd = self._device_D(D)
        kkt = None
        if hals and sl is not None:
            _, kkt = ops.hals_spatial_lists(A2, fp.packed_lists(floor=0.0), sl, A1, Cs, fp.sz_list, Dd, gamma, sweeps=sweeps,
                                            kkt=True, bbox=boxes)
        elif hals:
            _, kkt = ops.hals_spatial(A2, A1, Cs, Dd, gamma, sweeps=sweeps, boxes=boxes, kkt=True, sz=fp.sz_list)
        elif sl is not None:
            # the values and boxes of the true A (not the floored lists of K3n): a sub-floor value is updated like any other
            ops.mu_spatial_lists(A2, fp.packed_lists(floor=0.0), sl, A1, Cs, fp.sz_list, Dd, gamma)
        else:
            ops.mu_spatial(A2, A1, Cs, Dd, gamma)
        self.last_spatial_kkt = None if kkt is None else kkt.cpu()
        fp.A = A2.view(*fp.sz_list, K)
        self._footprints_written()
        return fp.A

    def _spatial_support(self, grow):
        """``(boxes, sl)`` of a 'hals' spatial_step: the (K,6) int32 boxes of the non-zero values of ``fp.A`` grown by ``grow``
        and clipped to the volume, and the tile lists made from them (None: the dense form, by the rule of ``_spatial_lists``).
        ``grow == 0``: the lists are the cached ones of the 'mu' path; else they are made here and kept nowhere."""
        fp = self.fp
        sz = fp.sz_list
        if fp.K <= LISTS_MAX_K:
            boxes = fp.packed_lists(floor=0.0)["bbox"]
        else:   # no list layout holds this many neurons: the same boxes from the values
            nz = fp.A.reshape(*sz, fp.K) != 0
            cols = []
            for ax in range(3):
                hit = nz.any(dim=tuple(a for a in range(3) if a != ax))      # (dim, K)
                at = torch.arange(sz[ax], device=hit.device)[:, None]
                cols += [torch.where(hit, at, sz[ax]).amin(0), torch.where(hit, at, -1).amax(0)]   # empty: lo > hi
            boxes = torch.stack(cols, 1).to(torch.int32).contiguous()
        g = [int(v) for v in grow] if hasattr(grow, "__len__") else [int(grow)] * 3
        if not any(g):
            return boxes, self._spatial_lists()
        boxes = ops.dilate_boxes(boxes, sz, g)
        if fp.P * 32 >= 2 ** 31 or sz[1] * sz[2] < 4:
            return boxes, None
        ext = (boxes[:, 1::2] - boxes[:, 0::2] + 1).clamp_min(0).long()
        if lists_verdict(self.spatial_kernel, fp.K, float(ext.prod(1).sum()) / fp.P) is not None:
            return boxes, None
        sl = ops.spatial_lists_setup({"bbox": boxes}, fp.K, sz)
        if sl["total"] <= 0:
            if self.spatial_kernel == 'lists':
                raise ValueError("spatial_kernel='lists': a tile lists more than 32 neurons (or none at all)")
            return boxes, None
        return boxes, sl

    def _spatial_numerator(self, registered, C, sl, A1, Cs, frame_ids, times):
        """K5 of spatial_step: the numerator into ``A1`` (compact sums at the listed entries when ``sl`` is given, else
        (P,K)) and ``C C^T`` of the local frames into ``Cs``."""
        if sl is not None:
            _, _, self._ws_k5 = ops.spatial_accum_lists(registered, C, sl, self.fp.sz_list, self.fp.K, frame_ids=frame_ids,
                                                        times=times, A1c=A1, Cs=Cs, workspace=self._ws_k5)
        else:
            self._spatial_accum_dense(registered, C, A1, Cs, frame_ids, times)

    def _scale_Cs(self, Cs):
        """spatial_step's hook on the all-reduced ``C C^T``, in place: nothing to do for one channel."""

    def _footprints_written(self):
        """K6 wrote ``fp.A`` through its raw pointer: every packed copy and tile list of the old footprints is stale."""
        self.fp.invalidate_layouts()
        self._sl = None

    def _spatial_buffer(self, n):
        """The one buffer of spatial_step (A1 | C_s: one collective), kept while its size holds."""
        if self._spatial_buf is None or self._spatial_buf.numel() != n:
            self._spatial_buf = None
            self._spatial_buf = torch.empty((n,), dtype=torch.float32, device=device)
        return self._spatial_buf

    @staticmethod
    def _spatial_accum_dense(registered, C, A1, Cs, frame_ids, times):
        """Dense K5 into A1 (P,K) and Cs (K,K): one launch up to 128 neurons, else columns of A1 by groups of 128 (K5 holds
        8 trace blocks per wave) and C C^T in float64 (it is tiny).  The frames of the call and their trace columns are
        those of ``ops._ids`` in both forms: as many as ``times``, else as ``frame_ids`` with column b for frame b, else every
        row of ``registered``."""
        K = C.shape[0]
        if K <= 128:
            ops.spatial_accum(registered, C, frame_ids=frame_ids, times=times, A1=A1, Cs=Cs, accumulate=False)
            return
        _, tt, B = ops._ids(registered, frame_ids, times, C.device)
        Cl = C[:, :B] if tt is None else C[:, tt.long()]
        for s0 in range(0, K, 128):
            part, _ = ops.spatial_accum(registered, C[s0:s0 + 128].contiguous(), frame_ids=frame_ids, times=times)
            A1[:, s0:s0 + 128] = part
        Cs.copy_((Cl.double() @ Cl.double().T).float())

    def _allreduce_spatial(self, buf):
        """Sum spatial_step's buffer over ``self.group`` when the T axis is sharded (nothing to do otherwise)."""
        if self.group is not None and torch.distributed.get_world_size(self.group) > 1:
            if self.collective == "c1" and torch.distributed.get_backend(self.group) == "nccl":
                # the library's own RCCL communicator (C1 of the C ABI: what a host without torch would call), built on
                # first use
                if self._comm is None:
                    self._comm = ops.Communicator(self.group)
                self._comm.all_reduce_(buf)
            else:  # the caller's process group: RCCL when its backend is "nccl" (one process per GPU), gloo in rehearsals
                with ops._timed("allreduce"):
                    torch.distributed.all_reduce(buf, group=self.group)

    def _device_D(self, D):
        """``D`` as fp32 (P,K) on the device, or None; the copy is kept while the caller hands in the same object (105 MB
        at cfg 3)."""
        if D is None:
            return None
        if self._D_dev is None or self._D_dev[0] is not D:
            self._D_dev = (D, torch.as_tensor(D).to(device, torch.float32).reshape(self.fp.P, self.fp.K).contiguous())
        return self._D_dev[1]

    def _spatial_lists(self):
        """Tile lists of the list-form footprint update (``ops.spatial_lists_setup``) when ``spatial_kernel`` allows it and
        the footprints are compact (the rule of the Gram kernel: few boxes per voxel; no tile with more than 32 neurons),
        else None: dense K5 / K6.  The boxes are those of every non-zero value, whatever ``fp.footprint_floor``."""
        fp = self.fp
        if fp.P * 32 >= 2 ** 31 or fp.sz_list[1] * fp.sz_list[2] < 4:
            return None
        ly, why = fp._lists_verdict(self.spatial_kernel, floor=0.0)
        if why is not None:
            return None
        # keyed on the layout itself: it is rebuilt whenever A is replaced, edited or invalidated
        if self._sl is None or self._sl[0] is not ly:
            self._sl = (ly, ops.spatial_lists_setup(ly, fp.K, fp.sz_list))
        sl = self._sl[1]
        if sl["total"] <= 0:
            if self.spatial_kernel == 'lists':
                raise ValueError("spatial_kernel='lists': a tile lists more than 32 neurons (or none at all)")
            return None
        return sl

    # ---- fit steps -------------------------------------------------------------------------------------
    def _gather_frames(self, loader):
        """All frames the loader yields, in its order, resident on the GPU as (T,P) plus their indices."""
        if isinstance(loader, ResidentLoader):
            return loader.frames_2d(), loader.order_tensor()
        staged = self._stage_epoch(loader) if self.stream_loader else None
        if staged is not None:
            order = torch.tensor([t for b in staged[1] for t in b], dtype=torch.int32)
            frames = staged[0]
            if staged[2]:   # the dataset's device frames, row t = frame t: in the loader's order
                n = order.numel()
                if n != frames.shape[0] or not bool((order == torch.arange(n, dtype=torch.int32)).all()):
                    frames = frames.index_select(0, order.to(device, torch.int64))
            return frames, order.to(device)
        fr, idx = [], []
        for data in loader:
            fr.append(data[0].to(device, torch.float32).reshape(data[0].shape[0], -1))
            idx.append(torch.as_tensor(data[1]).to(device, torch.int32).reshape(-1))
        return torch.cat(fr, 0).contiguous(), torch.cat(idx, 0)

    def _frames_in_time_order(self, loader):
        """``_gather_frames`` with the frames sorted by their times where the loader did not serve them so."""
        frames, order = self._gather_frames(loader)
        if not bool((order[1:] > order[:-1]).all()):
            at = torch.argsort(order.long())
            frames, order = frames.index_select(0, at), order[at]
        return frames, order

    def _residual_pieces(self, frames, order, C, registered, P):
        """The frames in pieces of at most 1 GiB -> per piece ``(s, fr, tt, sub)``: its first row, its frames (registered under
        the current ``fp.beta`` where ``registered`` says how), their times and the model's prediction ``fp.recon_image(C, tt)``
        as rows of ``P`` floats (None without ``C``)."""
        fp = self.fp
        step = _gib_rows(frames.shape[0], P)
        for s in range(0, frames.shape[0], step):
            fr, tt = frames[s:s + step], order[s:s + step]
            sub = None if C is None else ops.halo_interior(fp.recon_image(C, tt), fp.sz_list).reshape(fr.shape[0], P)
            if registered is not None:
                fr = fp.registered_video(fr, times=tt, interpolation=registered)
            yield s, fr, tt, sub

    def _single_model_only(self, who, loader=None, shard_reason=None):
        """The refusals of a step written for one channel and, with ``shard_reason`` (the text after ``who``), for a model and a
        loader that hold every frame."""
        if self._nchan() != 1:
            raise NotImplementedError(f"{who}: one channel only")
        sharded = self.group is not None or getattr(loader, "T_total", None) != getattr(loader, "T", None)
        if shard_reason is not None and sharded:
            raise NotImplementedError(f"{who}: {shard_reason}")

    def _box_sizes(self, who, boxes, what="neuron", hint="raise floor or lower margin"):
        """The voxels of each box (K,) int64; ValueError where one holds more than the box kernels take."""
        n = (boxes[:, 1::2] - boxes[:, 0::2] + 1).long().prod(1)
        if int(n.max()) > ops.COMPONENT_MAX_VOXELS:
            raise ValueError(f"{who}: the box of {what} {int(n.argmax())} holds {int(n.max())} voxels, at most "
                             f"{ops.COMPONENT_MAX_VOXELS} ({hint})")
        return n

    def _component_boxes(self, who, floor, margin):
        """``ops.component_boxes`` of the footprints, none larger than the box kernels take."""
        boxes = ops.component_boxes(self.fp.A.detach(), self.fp.sz_list, floor=floor, margin=margin)
        self._box_sizes(who, boxes)
        return boxes

    def _distance_prior(self, pos):
        """D = 1 - exp(-0.01 * distance(voxel, centre_k)) for the centres ``pos`` (n, 3), float64 numpy (P, n) (reference
        :133-137)."""
        d = torch.cdist(self.fp.flow_id.reshape(-1, 3).double(), pos.to(device).double())
        return (1 - torch.exp(-.01 * d)).cpu().numpy()

    def registered_video(self, loader, interpolation='linear', fill=None):
        """The motion-corrected movie of every frame ``loader`` serves, under the current ``fp.beta``: (T_loc, nchan*P) fp32
        CUDA rows in the loader's order (``ExponentialFP.registered_video``: ``'linear'`` = K17, trilinear in true voxel
        coordinates, an extension without the reference's ``sz``-for-``sz - 1`` quirk; ``'nearest'`` = K7, the reference's).
        ``self.last_registered_bad``: the number of lattice points the warp had no solution for (None for ``'nearest'``)."""
        with torch.no_grad():
            frames, order = self._gather_frames(loader)
            out = self.fp.registered_video(frames, times=order, interpolation=interpolation, fill=fill, nchan=self._nchan())
        bad = self.fp.last_registered_bad
        self.last_registered_bad = None if bad is None else int(bad)
        return out

    def summary_images(self, loader, source='video', registered=None, neighbours='full'):
        """The summary images (``ExponentialFP.summary_images``, K18) of every frame ``loader`` serves: a dict ``mean / std /
        max / corr`` of (X, Y, Z) float64 CUDA images.  ``source='residual'``: of Y - S_t with the model's reconstruction
        S_t = A C_t (``fp.recon_image``) -- where a neuron the model has no component for shows, which is how one sees that
        ``K`` was chosen too small; the kernel subtracts as it reads, no subtracted movie is made.  S_t lives in the
        coordinates of the footprints: with ``registered='linear'`` (K17) or ``'nearest'`` (K7) the frames are first
        registered to the footprint volume under the current ``fp.beta``, and the images are in the coordinates ``fp.A`` and
        ``detect_positions`` use; with ``registered=None`` the frames are taken as they are, which for the residual is right
        only where the warp is the identity.  The frames go through in pieces of at most 1 GiB."""
        if source not in ('video', 'residual'):
            raise ValueError(f"summary_images: source must be 'video' or 'residual', got {source!r}")
        if registered is not None:
            _check_registered(registered, "summary_images")
        self._single_model_only("summary_images")
        sz = self.fp.sz_list
        with torch.no_grad():
            frames, order = self._gather_frames(loader)      # in the loader's order, not sorted
            T = frames.shape[0]
            C = self.C.to(device, torch.float32).contiguous() if source == 'residual' else None
            state = images = None
            for s, fr, _, sub in self._residual_pieces(frames, order, C, registered, sz[0] * sz[1] * sz[2]):
                images, state = ops.summary_images(fr, sz, sub=sub, neighbours=neighbours, state=state, first=s == 0,
                                                   finish=s + fr.shape[0] >= T)
        return images

    def robust_images(self, loader, registered=None, **kw):
        """The order-statistic images (``ExponentialFP.robust_images``, K30; ``kw``: ``percentiles``, ``noise``) of every frame
        ``loader`` serves, in the loader's order: a dict of (X, Y, Z) float64 CUDA images.  ``registered='linear'`` (K17) or
        ``'nearest'`` (K7) registers the frames under the current ``fp.beta`` first, as ``summary_images`` does.  The selection
        sees the movie 9 times per group of quantiles (27 times in all with the defaults): the frames go through in pieces of at
        most 1 GiB each time, and registered frames are made anew each time.  One channel, and a loader that holds every frame."""
        if registered is not None:
            _check_registered(registered, "robust_images")
        self._single_model_only("robust_images", loader, "the loader holds a shard of the frames (a voxel's order statistics "
                                                         "need all of its samples)")
        sz = self.fp.sz_list
        with torch.no_grad():
            frames, order = self._gather_frames(loader)
            P = sz[0] * sz[1] * sz[2]
            return ops.robust_images(lambda: (fr for _, fr, _, _ in self._residual_pieces(frames, order, None, registered, P)), sz, **kw)

    def dff_movie(self, loader, registered=None, **kw):
        """The dF/F movie (``ExponentialFP.dff_movie``, K31; ``kw``: ``window``, ``stride``, ``percentile``, ``mode``, ``offset``,
        ``min_samples``) of every frame ``loader`` serves, in the order of the frame times: (T, P) fp32 CUDA rows.
        ``registered='linear'`` (K17) or ``'nearest'`` (K7) registers the frames under the current ``fp.beta`` first, as
        ``robust_images`` does.  The frames go through in pieces of at most 1 GiB that overlap by up to window - stride frames
        (registered frames of the overlap are made twice).  ``self.last_dff`` receives ``knots``, ``centres``, ``n``, ``starts``
        and ``ends``.  One channel, and a loader that holds every frame."""
        if registered is not None:
            _check_registered(registered, "dff_movie")
        self._single_model_only("dff_movie", loader, "the loader holds a shard of the frames (a running baseline needs the "
                                                     "frames next to each other)")
        percentile = float(kw.pop("percentile", 8.0))
        if not 0.0 <= percentile <= 100.0:
            raise ValueError(f"dff_movie: percentile must lie in [0, 100], got {percentile!r}")
        fp = self.fp
        with torch.no_grad():
            frames, order = self._frames_in_time_order(loader)

            def rows_of(r0, r1):
                if registered is None:
                    return frames[r0:r1]
                return fp.registered_video(frames[r0:r1], times=order[r0:r1], interpolation=registered)
            movie, info = ops.dff_rows(rows_of, frames.shape[0], fp.sz_list, kw.pop("window"), kw.pop("stride", None), percentile / 100.0,
                                       **kw)
        self.last_dff = info
        return movie

    def denoise_movie(self, loader, registered=None, **kw):
        """The movie of every frame ``loader`` serves, in the order of the frame times, denoised by local low-rank approximation
        (``ExponentialFP.denoise_movie``, K34; ``kw``: ``patch``, ``overlap``, ``rank``, ``keep``, ``threshold``, ``iters``,
        ``scale``): (T, P) fp32 CUDA rows.  ``registered='linear'`` (K17) or ``'nearest'`` (K7) registers the frames under the current
        ``fp.beta`` first, as ``robust_images`` does -- in frame coordinates a moving animal is not locally low-rank, so
        ``registered=None`` is for a movie that is static already.  The frames go through in pieces of at most 1 GiB, once per pass
        (registered frames are made anew each time).  ``self.last_denoise`` receives ``plan``, ``kept``, ``lam``, ``ok``,
        ``explained`` and the factors ``U``, ``Q``.  One channel, and a loader that holds every frame."""
        if registered is not None:
            _check_registered(registered, "denoise_movie")
        self._single_model_only("denoise_movie", loader, "the loader holds a shard of the frames (a patch's factors need all of "
                                                         "its frames)")
        fp = self.fp
        with torch.no_grad():
            frames, order = self._frames_in_time_order(loader)

            def rows_of(r0, r1):
                if registered is None:
                    return frames[r0:r1]
                return fp.registered_video(frames[r0:r1], times=order[r0:r1], interpolation=registered)
            movie, info = _denoise_rows(rows_of, frames.shape[0], fp.sz_list, kw.pop("scale", 'noise'), **kw)
        self.last_denoise = info
        return movie

    def detrend_traces(self, window, traces=None, **kw):
        """The traces read against their own running baseline (K31, ``Demix.Traces.detrend_df_f``; ``kw``: ``stride``,
        ``percentile``, ``mode``, ``offset``): ``self.C``, or ``traces`` (K, T) -- e.g. what ``clean_traces`` returned, whose NaN
        frames are left out of their windows -> (K, T) fp32 on the GPU.  ``self.C`` stays as it is; ``self.last_detrend``
        receives the ``baseline`` (K, T) of the call."""
        from .Traces import detrend_df_f
        self._single_model_only("detrend_traces", None, "the model holds a shard of the frames (a running baseline needs the "
                                                        "frames next to each other)")
        with torch.no_grad():
            C = (self.C if traces is None else torch.as_tensor(traces)).detach().to(device, torch.float32)
            out, baseline = detrend_df_f(C, window, **kw)
        self.last_detrend = dict(baseline=baseline)
        return out

    def evaluate_components(self, loader, registered='linear', active=0.25, margin=2, floor=1e-3, min_r=0.5, min_snr=1.0):
        """Which of the K components explain anything (K24, ``ops.component_stats``): one pass over the registered frames
        ``loader`` serves.  On the box of neuron k (``ops.component_boxes(fp.A, sz, floor, margin)``) and for frame t,
        e_t = Y_t - S_t + a_k C[k, t] -- the residual of the model S_t = A C_t (``fp.recon_image``) with the neuron's own
        contribution put back.  Returns, and stores in ``self.last_evaluation``, a dict of CUDA tensors:
        ``raw`` (K, n) the least-squares amplitude of a_k in e_t with a free offset, the neuron's raw trace, and ``frame_corr``
        (K, n) the Pearson correlation of a_k and e_t, per frame served in the order of the frame times; ``images`` (K, vmax)
        the mean of e_t over the neuron's ``n_active = ceil(active n)`` active frames, on its box (x slowest, NaN past the
        box); ``r_values`` (K) the Pearson correlation of a_k with that image; ``snr`` (K) = (mean of raw over the active
        frames - median of raw) / noise, noise = MAD(diff(raw)) / (0.6745 sqrt 2), the estimator ``deconvolve`` uses;
        ``boxes`` (K, 6) int32; ``keep`` (K) bool = ``r_values >= min_r`` and ``snr >= min_snr``, NaN failing
        (``select_components(keep)`` drops the others).
        The active frames of neuron k are those with the largest leave-one-out score (C[k, t-1] + C[k, t+1]) / 2 -- the one
        neighbour that exists at the two ends, ties to the earlier frame -- not those with the largest C[k, t]: the trace of a
        component on nothing is <a, noise_t> / |a|^2, so its largest entries pick the frames whose noise happens to look
        like a, and their mean image inherits the footprint's shape.  Calcium traces are correlated in time and the noise is
        not, so the neighbours find a real neuron's active frames and say nothing about the noise of frame t.
        ``min_r`` and ``min_snr`` are parameters, not tolerances: their defaults sit in the gap that a planted video of six
        cells and two components on nothing leaves between the two groups (tests/test_components_host.py measures it:
        r_values above 0.8 against below 0.3, snr above 2 against below 0.8).
        ``registered='linear'`` (K17, zero padding like ``summary_images``) or ``'nearest'`` (K7) registers the frames under
        the current ``fp.beta`` first; ``None`` takes them as they are, which is right only where the warp is the identity.  A
        frame with a sample that is not finite inside a neuron's box counts for nothing in that neuron's figures and is NaN
        in its ``raw`` and ``frame_corr``.  The frames go through in pieces of at most 1 GiB."""
        who = "evaluate_components"
        if registered is not None:
            _check_registered(registered, who)
        self._single_model_only(who, loader, "the loader holds a shard of the frames (the mean images would need an all-reduce)")
        if not 0 < active <= 1:
            raise ValueError(f"{who}: active={active!r} is the fraction of the frames that count as active, in (0, 1]")
        fp = self.fp
        sz, P, K = fp.sz_list, fp.P, fp.K
        with torch.no_grad():
            frames, order = self._frames_in_time_order(loader)
            T = frames.shape[0]
            C = self.C.to(device, torch.float32).contiguous()
            Cs = C[:, order.long()].contiguous()                     # the traces of the frames served, in time order
            A_rows = fp._layout("rows", (), lambda: fp.A.reshape(P, K).t().contiguous())
            boxes = self._component_boxes(who, floor, margin)
            score = Cs.double()
            if T > 1:
                score = torch.cat((Cs[:, 1:2], 0.5 * (Cs[:, :-2].double() + Cs[:, 2:].double()), Cs[:, -2:-1]), 1).double()
            n_active = min(T, max(1, int(math.ceil(active * T))))
            top = torch.sort(score, dim=1, descending=True, stable=True).indices[:, :n_active]
            w = torch.zeros((K, T), dtype=torch.float32, device=device).scatter_(1, top, 1.0)
            state, raw, corr = None, [], []
            for s, fr, _, sub in self._residual_pieces(frames, order, C, registered, P):
                e = s + fr.shape[0]
                out, state = ops.component_stats(fr, sz, A_rows, boxes, Cs[:, s:e], w[:, s:e], sub=sub, state=state, first=s == 0,
                                                 finish=e >= T)
                raw.append(out["raw"])
                corr.append(out["frame_corr"])
            raw, corr = torch.cat(raw, 1), torch.cat(corr, 1)
            snr = ops.component_snr(raw, w)
            keep = (out["r_values"] >= min_r) & (snr >= min_snr)     # a NaN compares False
        self.last_evaluation = dict(r_values=out["r_values"], snr=snr, frame_corr=corr, raw=raw, images=out["image"], boxes=boxes,
                                    n_active=n_active, keep=keep)
        return self.last_evaluation

    # what select_components forgets, with every last_* result: the caches and workspaces with a K-shaped extent
    _K_SHAPED = ("_ws_k2", "_ws_k3", "_S_bufs", "_S_zero", "_gram_nbr", "_sl", "_ws_k5", "_spatial_buf", "_ws_mg", "_D_dev")

    def _forget_k_shaped(self):
        """The tail of every call that changes the components: the packed layouts of ``fp.A``, the caches and workspaces with a
        K-shaped extent and every ``last_*`` result of an earlier call are forgotten."""
        self.fp.invalidate_layouts()
        for name in self._K_SHAPED + tuple(n for n in vars(self) if n.startswith("last_")):
            setattr(self, name, None)

    def _components_changed(self, K):
        """The model now holds ``K`` components: ``fp.K`` and ``K`` say so, and what ``_forget_k_shaped`` names is forgotten."""
        self.fp.K = K
        if hasattr(self, "K"):
            self.K = K
        self._forget_k_shaped()
        return K

    def select_components(self, keep):
        """Shrink the model in place to the neurons ``keep`` -- a bool mask (K,) or indices, e.g. ``evaluate_components(...)
        ['keep']`` -- in the order given (a mask: ascending): ``fp.A``, ``fp.pos``, ``fp.sigma``, ``fp.K``, ``C``, ``D`` and
        ``K``; ``fp.beta`` stays, the warp is shared.  Every packed layout, K-shaped cache and workspace and every
        ``last_*`` result of an earlier call is forgotten.  ValueError for an empty selection or an index out of range.
        Returns the number kept."""
        fp = self.fp
        K = fp.K
        sel = torch.as_tensor(keep).detach().cpu()
        if sel.dtype == torch.bool:
            if tuple(sel.shape) != (K,):
                raise ValueError(f"select_components: a mask must be ({K},), got {tuple(sel.shape)}")
            sel = torch.nonzero(sel).reshape(-1)
        elif sel.dtype.is_floating_point or sel.dim() != 1:
            raise ValueError("select_components: keep is a bool mask (K,) or a list of indices")
        sel = sel.long()
        if sel.numel() == 0:
            raise ValueError("select_components: the selection is empty")
        if int(sel.min()) < 0 or int(sel.max()) >= K:
            raise ValueError(f"select_components: index out of range for K={K}: {sel.tolist()}")
        self._single_model_only("select_components")
        with torch.no_grad():
            at = sel.to(fp.A.device)
            fp.A = fp.A.index_select(3, at).contiguous()
            fp.pos = fp.pos.index_select(0, at.to(fp.pos.device))
            fp.sigma = fp.sigma.index_select(0, at.to(fp.sigma.device))
            self.C = self.C.index_select(0, at.to(self.C.device)).contiguous()
            self.A = self.A.index_select(0, at.to(self.A.device))
        if self.D is not None:
            self.D = np.ascontiguousarray(self.D[..., sel.numpy()])
        return self._components_changed(int(sel.numel()))

    def merge_components(self, thr=0.85, min_overlap=0.1, floor=1e-3, margin=0, traces=None, iters=10, dry_run=False):
        """Merge the components that sit on one cell (K26; tests/merge_restatement.py is the definition).  The proposal step
        often yields two centres a voxel or two apart for one cell; both halves pass ``evaluate_components``, and their traces
        steal from each other.  Two components are joined when their boxes (``ops.component_boxes(fp.A, sz, floor, margin)``;
        margin 0: boxes that only touch through a margin are no candidates) intersect, the cosine of their footprints on the
        boxes' intersection is at least ``min_overlap`` and the Pearson correlation of their traces -- of ``traces`` (K, T)
        when given, e.g. what ``clean_traces`` or ``deconvolve`` returned, over the frames where both are finite; else of
        ``self.C`` -- is at least ``thr``; groups are the connected components of these edges.  A group becomes one
        component a' = sum u_k a_k, c' = sum w_k c_k, the rank-1 non-negative factor of sum_k a_k c_k^T (``ops.merge_plan``:
        ``iters`` alternating rounds in coefficient space, scaled to the norm of the dominant member); the merge always combines
        ``self.C``, whose merged rows must be finite and >= 0 (ValueError).  Its ``pos`` is the members' mean weighted by
        sqrt(|a_k|^2 |c_k|^2), its ``sigma`` and its row of ``self.A`` the dominant member's, its ``D`` the constructor's
        formula at the new ``pos``.
        The model shrinks in place as in ``select_components``: ``fp.A``, ``fp.pos``, ``fp.sigma``, ``fp.K``, ``C``, ``A``, ``D``
        and ``K`` are replaced, ``fp.beta`` stays, every packed layout, K-shaped cache and ``last_*`` result is forgotten.
        Returns, and stores in ``self.last_merge``, a dict: ``pairs`` (N, 2), ``overlap`` and ``corr`` (N,) CUDA tensors of the
        candidate pairs, ``groups`` a list of lists of old indices (ascending, ordered by their lowest member), ``merged`` the
        number of groups of two or more, ``K`` the new component count.  ``dry_run=True`` computes the dict and leaves the
        model bit for bit (``last_merge`` apart); so does a call in which nothing merges.
        ``thr`` and ``min_overlap`` are parameters, not tolerances: their defaults sit in the gap that a planted model of six
        cells leaves (tests/test_merge_host.py measures it, 24 x 20 x {1, 2}, T = 40, three seeds): the two halves of a split
        cell correlate at 0.981 or more and overlap at 0.946, distinct cells 1.5 sigma apart (overlap 0.34) with independent
        traces correlate at 0.75 or less, and cells that share a trace 8.6 voxels apart overlap at 0.016.
        The pair statistics run on the GPU; the groups and the coefficients are found on the host (a synchronisation: K is
        small).  One channel and one process only."""
        who = "merge_components"
        self._single_model_only(who, None, "the model holds a shard of the frames (the trace sums would need an all-reduce)")
        fp = self.fp
        sz, P, K = fp.sz_list, fp.P, fp.K
        with torch.no_grad():
            C = self.C.detach().to(device, torch.float32).contiguous()
            Ct = C
            if traces is not None:
                Ct = torch.as_tensor(traces).detach().to(device, torch.float32).contiguous()
                if tuple(Ct.shape) != tuple(C.shape):
                    raise ValueError(f"{who}: traces must be {tuple(C.shape)}, got {tuple(Ct.shape)}")
            A_rows = fp._layout("rows", (), lambda: fp.A.reshape(P, K).t().contiguous())
            boxes = self._component_boxes(who, floor, margin)
            stats = ops.component_pairs(A_rows, sz, boxes, Ct)
            groups = ops.merge_groups(stats, K, thr, min_overlap)
            merged = sum(len(g) >= 2 for g in groups)
            result = dict(pairs=stats["pairs"], overlap=stats["overlap"], corr=stats["corr"], groups=groups, merged=merged,
                          K=len(groups))
            if dry_run or merged == 0:
                self.last_merge = result
                return result
            rows = torch.tensor(sorted(k for g in groups if len(g) >= 2 for k in g), device=device)
            Cm = C.index_select(0, rows)
            if not bool((torch.isfinite(Cm) & (Cm >= 0)).all()):
                raise ValueError(f"{who}: the traces of the components to merge ({rows.tolist()}) have negative or non-finite "
                                 "entries: the rank-1 factor is defined for C >= 0")
            gstats = ops.component_pairs(A_rows, sz, boxes, C, pairs=ops.merge_group_pairs(groups))
            plan = ops.merge_plan(stats, K, thr, min_overlap, iters=iters, group_stats=gstats)
            A_new, C_new = ops.merge_apply(fp.A.reshape(P, K), C, plan)
            # what has one value per member: the weighted mean of pos, the dominant member's sigma and row of self.A
            seg = torch.repeat_interleave(torch.arange(len(groups)), torch.as_tensor(np.diff(plan["offsets"]).astype(np.int64)))
            wt = torch.from_numpy(plan["weight"])
            members = torch.from_numpy(plan["members"].astype(np.int64))
            pos_old = fp.pos.detach()
            num = torch.zeros((len(groups), 3), dtype=torch.float64).index_add_(0, seg, wt[:, None] * pos_old.cpu().double()[members])
            pos_new = num / torch.zeros(len(groups), dtype=torch.float64).index_add_(0, seg, wt)[:, None]
            dom = torch.from_numpy(plan["dominant"])
            single = torch.tensor([len(g) == 1 for g in groups])
            pos_new = pos_new.to(pos_old.dtype)
            pos_new[single] = pos_old.cpu()[dom[single]]              # an unmerged component keeps its bits
            fp.A = A_new.reshape(*sz, len(groups))
            fp.pos = pos_new.to(pos_old.device)
            fp.sigma = fp.sigma.index_select(0, dom.to(fp.sigma.device))
            self.C = C_new
            self.A = self.A.index_select(0, dom.to(self.A.device))
        if self.D is not None:
            D = np.ascontiguousarray(self.D[..., plan["dominant"]])
            for q in torch.nonzero(~single).reshape(-1).tolist():
                D[..., q] = self._distance_prior(fp.pos[q:q + 1]).reshape(*sz)
            self.D = D
        self._components_changed(len(groups))
        self.last_merge = result
        return result

    def clean_footprints(self, method='nrg', nrgthr=0.9999, maxthr=0.2, median=True, closing=True, values='filtered', floor=1e-3,
                         margin=1, dry_run=False):
        """Clean the learned footprints (K27; tests/footprint_clean_restatement.py is the definition, and ``ops.clean_footprints``
        has its bits).  An exact spatial solve (``spatial_solver='hals'`` with ``grow``) revives any voxel of a neuron's box
        where the noise happens to follow the trace: a learned footprint is then a cell plus isolated voxels, pinholes and
        sometimes a piece of a neighbour.  Per neuron, on its box (``ops.component_boxes(fp.A, sz, floor, margin)``; margin 1
        keeps the dilation from being clipped): the 3 x 3 x 3 median (``median``), the cut (``method='nrg'``: the largest values
        holding ``nrgthr`` of the energy; ``'max'``: above ``maxthr`` times the maximum), the closing (``closing``) and the
        largest face-connected part; the result holds the median (``values='filtered'``) or the learned values
        (``'original'``) on that part and 0 elsewhere.  Call it between sweeps, before ``evaluate_components`` or
        ``merge_components``.
        A neuron that cannot be cleaned -- no positive value or a non-finite one (it gets a one-voxel box), a negative value in
        its box, nothing left by the cut -- keeps its column bit for bit and has ``ok = 0``: the step never deletes a component.
        A box of more than 4096 voxels of a neuron with a positive value is a ValueError.
        ``fp.A`` is replaced in place; every packed layout, K-shaped cache and ``last_*`` result is forgotten as in
        ``select_components``; ``C``, ``pos``, ``sigma``, ``D`` and the warp stay.  Returns, and stores in
        ``self.last_footprint_clean``, a dict of (K,) CUDA tensors: int32 ``ok``, ``n_box``, ``n_cut``, ``n_closed``, ``n_parts``,
        ``n_kept``, float64 ``threshold`` and ``energy``, and ``boxes`` (K, 6) int32.  ``dry_run=True`` computes the dict and
        leaves the model bit for bit, ``last_footprint_clean`` included.  One channel and one process only."""
        who = "clean_footprints"
        self._single_model_only(who, None, "the model holds a shard of the frames (every rank would have to clean alike)")
        fp = self.fp
        sz, P, K = fp.sz_list, fp.P, fp.K
        with torch.no_grad():
            if not fp.A.is_contiguous():
                fp.A = fp.A.contiguous()
            A = fp.A.detach().view(P, K)
            boxes = ops.component_boxes(fp.A.detach(), sz, floor=floor, margin=margin)
            # a column that cannot be cleaned gets a one-voxel box that says so: its first value that is not finite, else, where
            # none is positive, the voxel 0
            odd = ~torch.isfinite(A)
            at = torch.where(odd.any(0), odd.to(torch.uint8).argmax(0), 0)
            hopeless = odd.any(0) | ~(A > 0).any(0)
            one = torch.stack((at // (sz[1] * sz[2]), at // sz[2] % sz[1], at % sz[2]), 1).repeat_interleave(2, 1).to(torch.int32)
            boxes = torch.where(hopeless[:, None], one, boxes)
            self._box_sizes(who, boxes)
            A_new, stats = ops.clean_footprints(A, sz, boxes, method=method, nrgthr=nrgthr, maxthr=maxthr, median=median,
                                                closing=closing, values=values, out=None if dry_run else A)
        result = dict(stats, boxes=boxes)
        if dry_run:
            return result
        self._forget_k_shaped()
        self.last_footprint_clean = result
        return result

    def add_components(self, loader, n, image='corr', registered='linear', shape_std=None, half=None, min_distance=None,
                       threshold=0.0, iters=5, min_explained=0.5, centres=None, dry_run=False):
        """Grow the model by the neurons it has no component for (K28; tests/add_restatement.py is the definition).  ``K`` is
        fixed at construction: a neuron that ``detect_positions`` missed on the template never enters the fit, and shows as a
        blob in ``summary_images(source='residual')``.  This call closes the loop without rebuilding the model.
        Candidates: up to ``n`` centres found by K14 (``ops.detect_neurons`` with ``shape_std`` -- default the median of
        ``fp.sigma`` --, ``min_distance`` -- default 2 ``shape_std`` -- and ``threshold``) in the residual summary image
        ``image`` (``'corr'``, ``'mean'``, ``'std'`` or ``'max'`` of ``summary_images(loader, 'residual', registered)``; a voxel
        that is NaN there gets the image's median); those within ``min_distance`` of an existing ``fp.pos`` are dropped.
        ``centres`` (M, 3) skips the detection and the drop: the caller's centres are taken as they are.
        Fit: the box of a candidate is its centre +- ``half`` voxels (``ops.candidate_boxes``; default ceil(2 ``shape_std``) per
        axis, 0 along an axis of extent 1), the start the model's Gaussian exp(-|u - centre|^2 / shape_std^2) on the box.  The
        frames ``loader`` serves go through K28a (``ops.residual_boxes``) in pieces of at most 1 GiB, registered first as in
        ``evaluate_components`` (``registered``), with the model's prediction ``fp.recon_image`` subtracted; K28b
        (``ops.rank1_nmf``, ``iters`` rounds) then factors every box's residual in one launch (candidates in batches whose
        residual stays within 1 GiB).  All candidates are fitted on the same residual, independently of each other -- not the
        sequential pick, fit, subtract of the greedy initialisers: two picks on one cell both come out as that cell and are
        left to ``merge_components``.
        A candidate is kept when its ``ok`` is set and ``explained / energy >= min_explained``: the share of its box's residual
        energy that a c^T takes off.  ``min_explained`` is a parameter, not a tolerance: its default sits in the gap that a
        planted video leaves (tests/test_add_host.py measures it, 24 x 20 x {1, 2}, T = 40, three seeds): the two cells the
        model lacks score 0.782 to 0.947 (their learned footprints correlate with the planted ones at 0.990 or more, the
        Gaussian start at 0.93), a box on nothing 0.076 or less.  A weak pick whose box takes in part of a missing cell is no
        box on nothing: it scores like the cell (0.89 and 0.90 measured where a noise peak lay 6 voxels from one), and is the
        case ``threshold`` or a following ``merge_components`` is for.
        For each candidate kept the model grows in place: ``fp.A`` gets a column (a scattered into a zero volume), ``fp.pos``
        the centre of mass of a, ``fp.sigma`` ``shape_std``, ``C`` a row (c at the times of the frames served; 0 at the others
        and on a frame with a sample that is not finite in the box), the unused ``self.A`` a zero row, ``D`` (when not None)
        the constructor's 1 - exp(-0.01 distance) in float64; ``fp.K`` and ``K`` go up, ``fp.beta`` stays.  Every packed
        layout, K-shaped cache and ``last_*`` result is forgotten as in ``select_components``.
        Returns, and stores in ``self.last_add``, a dict: ``centres`` (M, 3) float32 and ``boxes`` (M, 6) int32, float64
        ``explained`` and ``energy`` (M,), int32 ``ok`` (M,), bool ``kept`` (M,) -- CUDA tensors --, ``added`` their number and
        ``K`` the component count with them.  ``dry_run=True`` computes the dict and leaves the model bit for bit
        (``last_add`` apart); so does a call that keeps nothing.  One channel and one process only."""
        who = "add_components"
        self._single_model_only(who, loader, "the model or the loader holds a shard of the frames (every rank would have to add alike)")
        if int(n) < 1:
            raise ValueError(f"{who}: n={n!r} candidates, at least 1")
        if image not in ('corr', 'mean', 'std', 'max'):
            raise ValueError(f"{who}: image must be 'corr', 'mean', 'std' or 'max', got {image!r}")
        if registered is not None:
            _check_registered(registered, who)
        fp = self.fp
        sz, P, K = fp.sz_list, fp.P, fp.K
        sigma = float(fp.sigma.median()) if shape_std is None else float(shape_std)
        if not (sigma > 0.0 and math.isfinite(sigma)):
            raise ValueError(f"{who}: shape_std={shape_std!r} must be positive and finite")
        md = 2.0 * sigma if min_distance is None else float(min_distance)
        if half is None:
            half = [0 if s == 1 else int(math.ceil(2.0 * sigma)) for s in sz]
        with torch.no_grad():
            if centres is None:
                img = self.summary_images(loader, 'residual', registered)[image]
                img = torch.where(torch.isnan(img), torch.nanmedian(img), img).to(torch.float32).contiguous()
                pos, _, count = ops.detect_neurons(img, sz, int(n), shape_std=sigma, min_distance=md, threshold=threshold)
                cand = pos[:int(count)]
                if cand.shape[0]:
                    far = torch.cdist(cand.double(), fp.pos.detach().to(device).double()).amin(1) > md
                    cand = cand[far]
            else:
                cand = torch.as_tensor(centres).detach().to(device, torch.float32).reshape(-1, 3)
            M = cand.shape[0]
            f64 = dict(dtype=torch.float64, device=device)
            result = dict(centres=cand.contiguous(), boxes=torch.zeros((0, 6), dtype=torch.int32, device=device),
                          explained=torch.zeros(0, **f64), energy=torch.zeros(0, **f64),
                          ok=torch.zeros(0, dtype=torch.int32, device=device), kept=torch.zeros(0, dtype=torch.bool, device=device),
                          added=0, K=K)
            if M == 0:
                self.last_add = result
                return result
            boxes = ops.candidate_boxes(cand, sz, half)
            bh = boxes.cpu().numpy()
            ch = cand.cpu().numpy().astype(np.float64)
            nvox = self._box_sizes(who, boxes, "candidate", "lower half").cpu().numpy()
            vmax = int(nvox.max())
            # the start and the box coordinates on the host: M and vmax are small, and the centres had to come here anyway
            coords, a0 = [], np.zeros((M, vmax), dtype=np.float32)
            for m, b in enumerate(bh):
                g = np.meshgrid(*(np.arange(b[2 * d], b[2 * d + 1] + 1) for d in range(3)), indexing="ij")
                u = np.stack(g, -1).reshape(-1, 3).astype(np.float64)
                coords.append(u)
                a0[m, :u.shape[0]] = np.exp(-((u - ch[m][None, :]) ** 2).sum(1) / sigma ** 2)
            frames, order = self._frames_in_time_order(loader)
            T = frames.shape[0]
            if T > ops.ADD_MAX_FRAMES:
                raise ValueError(f"{who}: the loader serves {T} frames, at most {ops.ADD_MAX_FRAMES}")
            C = self.C.to(device, torch.float32).contiguous()
            batch = _gib_rows(M, T * vmax)
            fits = []
            for m0 in range(0, M, batch):
                E = torch.empty((min(batch, M - m0), T, vmax), dtype=torch.float32, device=device)
                for s, fr, _, sub in self._residual_pieces(frames, order, C, registered, P):
                    ops.residual_boxes(fr, sz, boxes[m0:m0 + batch], sub=sub, out=E, t0=s, n_total=T)
                fits.append(ops.rank1_nmf(E, nvox[m0:m0 + batch], torch.from_numpy(a0[m0:m0 + batch]).to(device), iters=iters))
                del E
            fit = {name: torch.cat([f[name] for f in fits], 0) for name in fits[0]}
            kept = (fit["ok"] == 1) & (fit["explained"] / fit["energy"] >= float(min_explained))     # a NaN compares False
            idx = torch.nonzero(kept).reshape(-1).tolist()
            result.update(boxes=boxes, explained=fit["explained"], energy=fit["energy"], ok=fit["ok"], kept=kept, added=len(idx),
                          K=K + len(idx))
            if dry_run or not idx:
                self.last_add = result
                return result
            ah = fit["a"].cpu().numpy()
            cols = torch.zeros((P, len(idx)), dtype=torch.float32, device=device)
            rows = torch.zeros((len(idx), C.shape[1]), dtype=torch.float32, device=device)
            com = np.zeros((len(idx), 3), dtype=np.float64)
            for q, m in enumerate(idx):
                am = ah[m, :nvox[m]].astype(np.float64)
                com[q] = (am[:, None] * coords[m]).sum(0) / am.sum()
                u = torch.from_numpy(coords[m].astype(np.int64)).to(device)
                cols[(u[:, 0] * sz[1] + u[:, 1]) * sz[2] + u[:, 2], q] = fit["a"][m, :nvox[m]]
                rows[q, order.long()] = torch.nan_to_num(fit["c"][m], nan=0.0)
            pos_new = torch.from_numpy(com).to(fp.pos.dtype)
            fp.A = torch.cat((fp.A.detach().reshape(P, K), cols), 1).reshape(*sz, K + len(idx)).contiguous()
            fp.pos = torch.cat((fp.pos.detach(), pos_new.to(fp.pos.device)), 0)
            fp.sigma = torch.cat((fp.sigma, torch.full((len(idx),), sigma, dtype=fp.sigma.dtype, device=fp.sigma.device)), 0)
            self.C = torch.cat((C, rows), 0).to(self.C.dtype)
            self.A = torch.cat((self.A, torch.zeros((len(idx),) + tuple(self.A.shape[1:]), dtype=self.A.dtype, device=self.A.device)), 0)
            if self.D is not None:
                self.D = np.concatenate((self.D, self._distance_prior(pos_new).reshape(*sz, len(idx))), -1)
        self._components_changed(K + len(idx))
        self.last_add = result
        return result

    def _background_refusals(self, loader, who):
        self._single_model_only(who, loader, "the loader holds a shard of the frames (the b step would need an all-reduce)")

    def update_background(self, loader, iters=3):
        """Fit the rank-1 background of the frames ``loader`` serves on what the current model leaves: Y_t ~ M_t + b f_t, with
        M_t the model's prediction in frame coordinates -- ``fp.recon_image`` followed by K2's warp, the forward of the motion
        loss -- and b >= 0 (X, Y, Z), f >= 0 one value per frame, by ``iters`` alternations of the two exact coordinate steps
        from b = 1 (K19, ``ops.background_fit``), scaled so that f has mean 1 over the frames served.  The kernels subtract M_t
        as they read; M_t is made piece by piece (at most 1 GiB of frames) and never held whole.  b lives in frame coordinates:
        camera offset, autofluorescence and out-of-focus glow do not move with the animal's neurons, and a static b needs no
        warp.  Stores and returns ``self.background = (b, f)``, fp32 CUDA, f (T,) indexed by frame time (0 for a frame the
        loader did not serve)."""
        return self._update_background(loader, iters, 1, 3, "update_background")

    def update_background_rank(self, loader, iters=3, rank=2, inner=3):
        """``update_background`` with R images and R time courses (K23, ``ops.background_fit_rank``), 2 <= R <= 8: Y_t ~ M_t +
        sum_j b_j f_j[t], b (R, X, Y, Z) and f (R, T), each f_j of mean 1 over the frames served; ``inner``: the coordinate sweeps
        per frame and per voxel of every half-step.  The time courses start as the indicators of R contiguous blocks of the
        frame times, so the frames go through in the order of their times.  ``rank=1`` is ``update_background(loader, iters)``,
        whatever ``inner`` is."""
        return self._update_background(loader, iters, rank, inner, "update_background_rank")

    def _update_background(self, loader, iters, rank, inner, who):
        self._background_refusals(loader, who)
        if int(rank) != rank or not 1 <= rank <= ops.BACKGROUND_RANKS[1]:
            raise ValueError(f"{who}: rank={rank!r} (1 .. {ops.BACKGROUND_RANKS[1]})")
        fp = self.fp
        sz, P = fp.sz_list, fp.P
        with torch.no_grad():
            frames, order = self._frames_in_time_order(loader) if rank > 1 else self._gather_frames(loader)
            if rank > max(1, order.numel()):
                raise ValueError(f"{who}: rank={rank} for the {order.numel()} frames served")
            C = self.C.to(device, torch.float32).contiguous()
            beta = fp.beta.detach()
            piece = min(_gib_rows(frames.shape[0], P), K2_MAX_FRAMES)
            zeros = torch.zeros((piece, P), dtype=torch.float32, device=device)

            def predict(s, e):
                tt = order[s:e]
                out = ops.warp_recon_grad(fp.recon_image(C, tt), None, None, None, sz, beta, tt, grad=None, gout=zeros[:e - s],
                                          want_recon=True, want_loss=False, want_reg=False, workspace=self._ws_k2)
                self._ws_k2 = out["workspace"]
                return out["recon"]

            if rank == 1:
                b, f_served = ops.background_fit(frames, sz, iters, sub_fn=predict, piece=piece)
            else:
                b, f_served = ops.background_fit_rank(frames, sz, iters, rank, sub_fn=predict, piece=piece, inner=inner)
            f = torch.zeros(f_served.shape[:-1] + (fp.T,), dtype=torch.float32, device=device)
            f[..., order.long()] = f_served
        self.background = (b, f)
        return self.background

    def background_loader(self, loader):
        """A ``ResidentLoader`` over ``max(Y_t - b f_t, 0)``, the frames of ``loader`` without the fitted background
        (``update_background``; ValueError before one was fitted; ``max(Y_t - sum_j b_j f_j[t], 0)`` for one of rank R).  The clamp is there because the multiplicative updates need
        Y >= 0, as the datasets' own clamp does.  It keeps the loader's batch size, shuffle flag, generator and volume, and
        serves frame t as row t: a ``ResidentLoader`` or a ``DataLoader`` whose pass covers the frames 0 .. n-1."""
        if self.background is None:
            raise ValueError("background_loader: no background was fitted (update_background)")
        self._background_refusals(loader, "background_loader")
        b, f = self.background
        batch_size = getattr(loader, "batch_size", None)
        if not batch_size:
            raise ValueError("background_loader: the loader has no batch_size (a ResidentLoader or a DataLoader)")
        if isinstance(loader, ResidentLoader):
            shuffle, generator = loader.shuffle, loader.generator
        else:
            from torch.utils.data import RandomSampler
            sampler = getattr(loader, "sampler", None)
            shuffle = isinstance(sampler, RandomSampler)
            generator = getattr(sampler, "generator", None) or getattr(loader, "generator", None)
        with torch.no_grad():
            frames, order = self._gather_frames(loader)
            n = order.numel()
            if isinstance(loader, ResidentLoader):
                rows = ops.background_subtract(frames, b, f, times=order)
            else:
                at = torch.argsort(order.long())
                if not bool((order[at].long() == torch.arange(n, device=order.device)).all()):
                    raise ValueError("background_loader: one pass of the loader must serve the frames 0 .. n-1 once each")
                rows = ops.background_subtract(frames, b, f, frame_ids=at, times=order[at])
        return ResidentLoader(rows, self.fp.sz_list, batch_size, shuffle=shuffle, generator=generator)

    def clean_traces(self, fps, **kw):
        """The traces ``self.C`` cleaned up for plotting and analysis (K20, ``ops.clean_traces``; the reference's
        ``Demix/Traces.py::cleanTraces``): acquisition outliers masked, single-frame jumps removed, every neuron's own bleaching
        detrended, scaled to [0.05, 0.95] or to dF/F0 -> ``(traces (K, T) fp32, scales (K,), offsets (K,))`` on the GPU.  ``fps``:
        frames per second; ``kw``: ``sigma_threshold``, ``detrend_mode``, ``interp_method``, ``smooth_method``, ``smooth_window``,
        ``trim``, ``floor``.  ``self.C`` stays as it is; ``self.last_clean`` receives the per-neuron ``a``, ``b``, ``F0``, ``fitted``
        and ``n_outliers`` of the call."""
        with torch.no_grad():
            C = self.C.detach().to(device, torch.float32)
            out, scales, offsets, info = ops.clean_traces(C if C.stride(-1) == 1 else C.contiguous(), fps, **kw)
        info.pop("workspace")
        self.last_clean = info
        return out, scales, offsets

    def deconvolve(self, fps=None, decay_time=None, traces=None, **kw):
        """When each neuron fired (K21, ``Demix.Traces.deconvolveTraces``): the AR(1), non-negative deconvolution of ``self.C``, or
        of ``traces`` (K, T) -- e.g. what ``clean_traces`` returned, whose NaN frames carry no weight -> ``(c, s, info)`` on the GPU:
        the denoised traces, the spikes and the per-neuron ``g``, ``penalty``, ``baseline``, ``noise``, ``rss``, ``n_valid``,
        ``n_pools`` and ``ok``.  ``decay_time`` in seconds needs ``fps``; ``kw``: ``g``, ``penalty``, ``baseline``, ``noise``,
        ``baseline_percentile``.  ``self.C`` stays as it is; ``self.last_deconv`` receives ``info``."""
        from .Traces import deconvolveTraces
        with torch.no_grad():
            C = (self.C if traces is None else torch.as_tensor(traces)).detach().to(device, torch.float32)
            c, s, info = deconvolveTraces(C, fps=fps, decay_time=decay_time, **kw)
        self.last_deconv = info
        return c, s, info

    def match_traces(self, reference, nbins=100, type='regular', traces=None):
        """The traces in the units of ``reference`` (K25, ``Demix.Traces.histogram_match``): NMF leaves the scale of every trace
        arbitrary, and per neuron the affine map that carries the quantiles of its trace onto those of its reference puts the two
        in the same units -- robust to a few wild frames, and without a frame-to-frame correspondence.  Matches ``self.C``, or
        ``traces`` (K, T) -- e.g. what ``clean_traces`` returned, whose NaN frames count for nothing.  ``reference``: (K, T') or
        (T',), one for all -- ROI traces from ``roi_signals``, another channel's traces, ground truth; array or tensor ->
        the matched traces (K, T) fp32 on the GPU.  ``type``: 'regular' or 'non-negative' (both coefficients >= 0).  ``self.C``
        stays as it is; ``self.last_match`` receives ``beta`` (K, 2: scale, offset), ``distance`` (K,) and ``ok`` (K,) of the
        call."""
        if type not in ("regular", "non-negative"):
            raise ValueError(f"match_traces: type={type!r}: 'regular' or 'non-negative'")
        with torch.no_grad():
            C = (self.C if traces is None else torch.as_tensor(traces)).detach().to(device, torch.float32)
            ref = torch.as_tensor(reference).detach().to(device, torch.float32)
            out, beta, distance, info = ops.histogram_match(C if C.stride(-1) == 1 else C.contiguous(),
                                                            ref if ref.stride(-1) == 1 else ref.contiguous(), nbins,
                                                            nonneg=type == "non-negative")
        self.last_match = dict(beta=beta, distance=distance, ok=info[:, 2] != 0)
        return out

    def update_footprints(self, testloader, batch_size, sz, gamma_c=1e-2, gamma_a=1e0, iter_c=10, return_dense=None,
                          live_spatial=False, iter_a=1, solver='mu', registered='nearest', spatial_solver='mu', grow=0,
                          ar_g=None, ar_penalty=0.0, ar_baseline=0.0):
        """Reference :163-179: ``iter_c`` multiplicative updates of ``self.C`` under the current warp.

        ``solver='ar1'`` (extension, K32) puts the calcium dynamics into the fit: ``iter_c`` sweeps of block coordinate descent
        over the neurons from the same ``self.C``, on the same Gram data (the dense path, frames sorted by time), each row
        replaced by the AR(1), non-negative deconvolution of its own residual trace weighted by ``G_t[k,k]``
        (``ops.ar1_temporal``; tests/ar1_restatement.py is the definition).  ``ar_g``: the decay per frame, a number or (K,);
        None estimates it per neuron from the current traces with K21's estimator, and a trace that cannot be treated gets 0,
        the plain non-negative step.  ``ar_penalty`` >= 0 and ``ar_baseline``: a number or (K,).  Needs ``gamma_c == 0`` (the
        AR model replaces that term), frame times that are a run of consecutive integers, at most 6144 of them, one channel and
        a model and loader that hold every frame.  ``self.last_temporal_ar`` then holds ``g``, ``penalty``, ``baseline``, ``s``
        (K, T; the spikes, in time order), ``colour``, ``n_colours``, ``n_pools``, ``n_weightless`` and ``F``, the objective
        before the call and after it (float64, the state before ``self.C`` is rounded to float32; it does not rise from traces
        that meet the constraints, while a start below the baseline or falling faster than ``g`` is no admissible point and may
        lie lower); ``last_temporal_kkt`` is None.

        ``solver='hals'`` (extension) runs ``iter_c`` sweeps of the exact solver K4h instead, from the same ``self.C``, on
        the same Gram data: cyclic coordinate descent on the non-negative least-squares problem the multiplicative update
        only approaches (with ``gamma_c != 0`` red-black over the frames).  ``self.last_temporal_kkt`` then holds, per frame
        of the call, how far the solver's float64 state was from that problem's solution after the last sweep (largest
        projected-gradient entry) -- the state BEFORE ``self.C`` is rounded to float32: it falls to ~1e-15 of the gradient's
        terms with enough sweeps, while the stored float32 traces sit at their rounding floor, ~1e-7
        (``ops.hals_temporal_kkt`` on ``self.C`` gives that figure).

        Returns ``(A_t, Y_i, Y)`` like the reference when the dense float64 ``A_t`` fits
        ``DENSE_RETURN_LIMIT`` (or ``return_dense=True``); otherwise ``(None, None, None)``.
        ``Y_i`` comes from the nearest-neighbour search K7 (``dnmf_image_iwarp``) unless ``registered='linear'``.
        ``gamma_a`` is unused unless ``live_spatial`` is set, as in the reference (its footprint update is commented
        out, :174).  ``live_spatial=True`` (extension) wires that update: after the temporal updates the frames are
        registered (K7) and ``fp.A`` takes ``iter_a`` multiplicative updates ``A * (Y_i C^T) / (A C C^T + gamma_a D +
        1e-32)`` (``spatial_step``: K5, one all-reduce over ``self.group``, K6) with the ``D`` of the constructor
        flattened over the voxels -- the reference's commented lines update an unrelated random ``self.A`` with
        mismatched shapes (:131, :169-176); here the update acts on the footprints the model uses.
        ``spatial_solver='hals'`` (extension): ONE ``spatial_step(solver='hals', sweeps=iter_a, grow=grow)`` instead -- one
        registration and one K5 pass over the movie, then ``iter_a`` sweeps of the exact solver K6h on supports grown by
        ``grow`` voxels; ``self.last_spatial_kkt`` (K,) holds its per-neuron distance from the solution (None after 'mu').

        ``registered='linear'`` (extension) registers with K17 (``ops.warp_pullback``: trilinear, true voxel coordinates,
        without the reference's ``sz``-for-``sz - 1`` quirk -- not a parity path) instead of K7, both for the ``live_spatial``
        input of ``spatial_step`` and for the returned ``Y_i``; the default ``'nearest'`` is the reference's."""
        fp = self.fp
        K, P = fp.K, fp.P
        _check_trace_solver(solver)
        _check_registered(registered, "update_footprints")
        _check_spatial_solver(spatial_solver, iter_a if spatial_solver == 'hals' else 1, grow, "update_footprints")
        hals, ar1 = solver == 'hals', solver == 'ar1'
        if hals:
            _hals_refuse_shards(gamma_c, self.group)
        if ar1:
            self._ar1_refusals(testloader, gamma_c)
        with torch.no_grad():
            frames, order = self._frames_in_time_order(testloader) if ar1 else self._gather_frames(testloader)
            if ar1 and not bool((order[1:] - order[:-1] == 1).all()):
                raise ValueError("update_footprints(solver='ar1'): the frame times must be a run of consecutive integers "
                                 "(the AR(1) model links every frame to the one before)")
            T_loc = frames.shape[0]
            Csel = self.C.to(device, torch.float32)[:, order.long()].contiguous()
            ly = None if ar1 else self._lists_layout_for_fused_update(gamma_c)
            kkt = None
            if ly is not None:
                # K3n leaves its slot tables in the workspace and K4 / K4h reads them there: no dense (T,K,K) in between
                _, _, self._ws_k3 = ops.warp_gram_rhs_lists(ly, K, fp.sz_list, fp.beta.detach(), order, frames,
                                                            workspace=self._ws_k3, finish=False)
                if hals:
                    Cnew, kkt = ops.hals_temporal_slots(ly, self._ws_k3, fp.sz_list, Csel.clone(), iter_c, kkt=True)
                else:
                    Cnew = ops.mu_temporal_slots(ly, self._ws_k3, fp.sz_list, Csel.clone(), iter_c)
            else:
                G, r = self._gram_rhs(frames, order)
                if ar1:
                    Cnew = self._ar1_temporal(G, r, Csel, iter_c, ar_g, ar_penalty, ar_baseline)
                elif hals:
                    Cnew, kkt = _hals_temporal(G, r, Csel, gamma_c, iter_c, group=self.group, nbr=self._gram_nbr)
                else:
                    Cnew = _mu_temporal(G, r, Csel, gamma_c, iter_c, group=self.group, nbr=self._gram_nbr)
            self.last_temporal_kkt = None if kkt is None else kkt.cpu()
            if not ar1:
                self.last_temporal_ar = None
            if hals and self.verbose:
                print('Temporal KKT: max %.3e median %.3e' % (float(self.last_temporal_kkt.max()),
                                                              float(self.last_temporal_kkt.median())))
            C = self.C.to(device, torch.float32).clone()
            C[:, order.long()] = Cnew
            self.C = C
            if live_spatial:
                nch = self._nchan()   # channels share the warp: one K7 search per lattice point serves all of them
                if self._reg_buf is None or self._reg_buf.shape != (T_loc, nch * P):
                    self._reg_buf = None
                    self._reg_buf = torch.empty((T_loc, nch * P), dtype=torch.float32, device=device)
                if registered == 'linear':
                    ops.warp_pullback(frames, None, fp.sz_list, fp.beta.detach(), order, out=self._reg_buf, nchan=nch)
                else:
                    ops.image_iwarp(frames, None, fp.sz_list, fp.beta.detach(), order, out=self._reg_buf, nchan=nch)
                if spatial_solver == 'hals':
                    self.spatial_step(self._reg_buf, D=self.D, gamma=gamma_a, times=order, solver='hals', sweeps=iter_a, grow=grow)
                    if self.verbose:
                        print('Spatial KKT: max %.3e median %.3e' % (float(self.last_spatial_kkt.max()),
                                                                     float(self.last_spatial_kkt.median())))
                else:
                    for _ in range(iter_a):
                        self.spatial_step(self._reg_buf, D=self.D, gamma=gamma_a, times=order)
            if return_dense is None:
                return_dense = 8 * P * K * T_loc <= DENSE_RETURN_LIMIT
            if not return_dense:
                return None, None, None
            X, Y_, Z = fp.sz_list
            A_t = np.empty((X, Y_, Z, K, T_loc))
            step = max(1, int((256 << 20) // (4 * P * K)))
            for s in range(0, T_loc, step):
                a, _ = ops.warp_gather(fp.A.contiguous(), fp.beta.detach(), order[s:s + step], want_grid=False)
                A_t[..., s:s + step] = a.permute(2, 3, 4, 1, 0).double().cpu().numpy()
            Yv = frames.view(T_loc, X, Y_, Z).permute(1, 2, 3, 0).double().cpu().numpy()
            Yi = np.empty_like(Yv)
            for s in range(0, T_loc, 256):
                if registered == 'linear':
                    yi = ops.warp_pullback(frames[s:s + 256], None, fp.sz_list, fp.beta.detach(), order[s:s + 256])
                else:
                    yi = ops.image_iwarp(frames, order[s:s + 256], fp.sz_list, fp.beta.detach(), order[s:s + 256])
                Yi[..., s:s + 256] = yi.view(-1, X, Y_, Z).permute(1, 2, 3, 0).double().cpu().numpy()
            return A_t, Yi, Yv

    def _ar1_refusals(self, loader, gamma_c):
        """What ``update_footprints(solver='ar1')`` does not take: the smoothing term, several channels, a sharded time axis."""
        who = "update_footprints(solver='ar1')"
        if not (gamma_c is None or gamma_c == 0):
            raise ValueError(f"{who}: gamma_c={gamma_c!r}: the AR(1) model replaces the smoothing term, pass gamma_c=0")
        if self._nchan() != 1:
            raise ValueError(f"{who}: one channel only (MultiChannelDNMF is not supported)")
        if self.group is not None or getattr(loader, "T_total", None) != getattr(loader, "T", None):
            raise ValueError(f"{who}: a model or loader sharded over ranks is not supported: the row step needs every frame of "
                             "a neuron's trace in one place")

    def _ar1_temporal(self, G, r, Csel, sweeps, ar_g, ar_penalty, ar_baseline):
        """``sweeps`` sweeps of K32 from ``Csel`` (K, T) fp32, the frames in time order, on the dense Gram data -> the new traces;
        fills ``self.last_temporal_ar``."""
        if G.shape[0] > ops.AR1_MAX_FRAMES or G.shape[1] > ops.AR1_MAX_K:
            raise ValueError(f"update_footprints(solver='ar1'): K={G.shape[1]}, T={G.shape[0]}: at most {ops.AR1_MAX_K} neurons "
                             f"and {ops.AR1_MAX_FRAMES} frames")
        if ar_g is None:
            est = ops.deconvolve_traces(Csel, penalty=0.0, baseline=0.0)[2]
            ar_g = torch.where(est["ok"], est["g"], torch.zeros_like(est["g"]))
        f0 = _ar1_objective(G, r, Csel.double(), ar_g, ar_penalty, ar_baseline)
        Cnew, s, info = ops.ar1_temporal(G, r, Csel.clone(), ar_g, ar_penalty, ar_baseline, sweeps=sweeps, nbr=self._gram_nbr)
        f1 = _ar1_objective(G, r, info["state"], ar_g, ar_penalty, ar_baseline)
        K = Cnew.shape[0]
        per = lambda v: torch.as_tensor(v, dtype=torch.float64).detach().cpu().expand(K).clone()   # noqa: E731
        self.last_temporal_ar = dict(g=per(ar_g), penalty=per(ar_penalty), baseline=per(ar_baseline), s=s, colour=info["colour"],
                                     n_colours=info["n_colours"], n_pools=info["n_pools"].cpu(),
                                     n_weightless=info["n_weightless"].cpu(), F=(f0, f1))
        if self.verbose:
            print('AR(1) temporal: F %.6e -> %.6e, %d colours' % (f0, f1, info["n_colours"]))
        return Cnew

    def _lists_layout_for_fused_update(self, gamma_c):
        """The K3n layout when update_footprints can run as K3n + K4-on-slots (one channel, no neighbour term, the
        kernel choice allows K3n and the pattern is narrow enough for the per-row lists); else None."""
        if not (gamma_c is None or gamma_c == 0) or len(self._channels()) != 1:
            return None
        ly, why = self.fp._lists_verdict(self.gram_kernel, slots=True, nbr=True)
        return ly if why is None else None

    def _gram_rhs(self, frames, order):
        """Per-frame Gram matrices and right-hand sides under the current warp, summed over the channels."""
        G = r = None
        chans = self._channels()
        self._gram_nbr = None
        for fp, cols in chans:
            Gc, rc = self._gram_rhs_one(fp, frames if cols is None else frames[:, cols], order)
            G, r = (Gc, rc) if G is None else (G.add_(Gc), r.add_(rc))
        if len(chans) > 1:
            self._gram_nbr = None   # the channels' patterns may differ
        return G, r

    def _channels(self):
        """``[(spatial model, slice of a frame row)]``: one entry, the whole row, for the reference's single-channel
        model; MultiChannelDNMF lists its colour channels here."""
        return [(self.fp, None)]

    def _nchan(self):
        """Channels of a frame row (P floats each)."""
        return 1

    def _note_once(self, key, text):
        """One line on stdout the first time ``key`` comes up (kernel choices that cost a factor and would otherwise
        go unnoticed)."""
        if key not in self._warned:
            self._warned.add(key)
            print("[dnmf_amd] " + text, flush=True)

    def _gram_rhs_one(self, fp, frames, order):
        """K3, K3s or K3n on the footprints of ``fp``."""
        ly, why = fp._lists_verdict(self.gram_kernel, slots=True)
        if why is None:
            G, r, self._ws_k3 = ops.warp_gram_rhs_lists(ly, fp.K, fp.sz_list, fp.beta.detach(), order, frames,
                                                        workspace=self._ws_k3)
            self._gram_nbr = ly["nbr"]   # the pattern of this G, for K4
            return G, r
        if self.gram_kernel == 'lists' and why == 'slots':
            raise ValueError(f"gram_kernel='lists': the pattern of G has {ly['nslot']} slots > "
                             f"{ops.LISTS_MAX_SLOTS} (footprints overlap too much)")
        if self.gram_kernel == 'auto' and why == 'K':
            self._note_once("k3n-K", f"gram_kernel='auto': K={fp.K} > {LISTS_MAX_K}, the neuron-list kernel K3n does not "
                            "apply; using K3s / K3 by pairs of neuron groups (several times slower)")
        elif self.gram_kernel == 'auto':   # 'slots' or 'boxes'
            self._note_once("k3n-shape", f"gram_kernel='auto': footprints too wide for the neuron-list kernel K3n "
                            f"(pattern slots {ly['nslot']} vs limit {ops.LISTS_MAX_SLOTS}, mean boxes per voxel "
                            f"{ly['boxfrac']:.2f} vs limit {LISTS_BOXFRAC_LIMIT}); using K3s / K3 (6-40x slower)")
        if fp.K > 127:
            return self._gram_rhs_grouped(fp, frames, order)
        sp = fp.packed_sparse() if self.gram_kernel in ('auto', 'sparse') else None
        if sp is not None and (self.gram_kernel == 'sparse' or sp["occupancy"] < 0.5):
            G, r, self._ws_k3 = ops.warp_gram_rhs_sparse(sp["Aps"], fp.K, sp["order"], sp["row_mask"], fp.sz_list,
                                                         fp.beta.detach(), order, frames, workspace=self._ws_k3)
        else:
            G, r, self._ws_k3 = ops.warp_gram_rhs(fp.packed_footprints(), fp.K, fp.sz_list, fp.beta.detach(), order,
                                                  frames, workspace=self._ws_k3, bf16=self.gram_kernel == 'bf16')
        return G, r

    def _gram_rhs_grouped(self, fp, frames, order):
        """K > 127: one launch holds at most 8 blocks of 16 channels, so the neurons are cut into groups and every
        PAIR of groups is one launch on their union; the launch yields both diagonal blocks and the off-diagonal
        block of the pair (diagonal blocks are recomputed by every pair they belong to).  K3s (groups of 64 along
        the Z-order curve) unless ``gram_kernel == 'dense'`` or the footprints are dense (K3, groups of 56)."""
        K, B = fp.K, order.numel()
        G = torch.empty((B, K, K), dtype=torch.float32, device=device)
        r = torch.empty((B, K), dtype=torch.float32, device=device)

        def sparse(pair):
            cols, sp = pair
            Gp, rp, self._ws_k3 = ops.warp_gram_rhs_sparse(sp["Aps"], cols.numel(), sp["order"], sp["row_mask"], fp.sz_list,
                                                           fp.beta.detach(), order, frames, workspace=self._ws_k3)
            return cols, Gp, rp

        def dense(cols):
            Gp, rp, self._ws_k3 = ops.warp_gram_rhs(fp.packed_columns(cols), len(cols), fp.sz_list, fp.beta.detach(), order,
                                                    frames, workspace=self._ws_k3, bf16=self.gram_kernel == 'bf16')
            return torch.as_tensor(cols, device=device), Gp, rp

        pairs = fp.packed_sparse_pairs() if self.gram_kernel in ('auto', 'sparse') else None
        if pairs is not None and (self.gram_kernel == 'sparse' or max(sp["occupancy"] for _, sp in pairs) < 0.5):
            _gram_by_pairs(G, r, pairs, sparse)
        else:
            _gram_by_pairs(G, r, _dense_unions(K), dense)
        return G, r

    def _recon_cache(self):
        """Reconstruction images S_t = A.C_t of all T frames, one (T,lds) tensor per channel (C is constant inside
        update_motion); None when they do not fit ``RECON_CACHE_LIMIT``."""
        chans = self._channels()
        fp0 = chans[0][0]
        lds = ops.halo_voxels(fp0.sz_list)
        if 4 * lds * fp0.T * len(chans) > RECON_CACHE_LIMIT:
            return None
        C = self.C.to(device, torch.float32).contiguous()
        all_t = torch.arange(fp0.T, dtype=torch.int32, device=device)
        # the buffers are kept between calls: re-allocating gigabytes every epoch makes the caching allocator split and
        # re-map its large blocks (tens of milliseconds every few sweeps)
        if self._S_bufs is None or len(self._S_bufs) != len(chans) or self._S_bufs[0].shape != (fp0.T, lds):
            self._S_bufs = [torch.empty((fp0.T, lds), dtype=torch.float32, device=device) for _ in chans]
            self._S_zero = [[None] for _ in chans]
        out = []
        for (fp, _), S, zs in zip(chans, self._S_bufs, self._S_zero):
            # every row is rewritten on every call; tiles no neuron reaches were zeroed by the first call with these
            # footprints and are skipped from then on (a third of the tiles -- and of the stores -- at 512x512, K = 100)
            was = zs[0]
            for s in range(0, fp.T, 32768):
                state = [was]
                fp.recon_image(C, all_t[s:s + 32768], out=S[s:s + 32768], zero_state=state)
            zs[0] = state[0]
            out.append(S)
        return out

    def _k2(self, S_all, Cdev, frames, frame_ids, times, grad, norm, want):
        """K2 for one set of frames on every channel: ``grad`` (10,3,T) is incremented by d mse / d beta, the mean
        running over ``norm`` frames (0 = all of ``times``) x channels x voxels.  Returns the outputs of
        ``ops.warp_recon_grad`` with the losses summed over channels."""
        chans = self._channels()
        nc = len(chans)
        if (nc > 1 or times.numel() > K2_MAX_FRAMES) and norm == 0:
            norm = times.numel()
        if times.numel() > K2_MAX_FRAMES:
            # frames ride on gridDim.y (<= 65535): larger sets go in pieces; grad accumulates, columns are independent
            total = None
            for s in range(0, times.numel(), K2_MAX_FRAMES):
                e = s + K2_MAX_FRAMES
                out = self._k2(S_all, Cdev, frames if frame_ids is not None else frames[s:e],
                               None if frame_ids is None else frame_ids[s:e], times[s:e], grad, norm, want)
                if total is None:
                    total = out
                elif want:
                    total["loss"] = total["loss"] + out["loss"]
                    total["frame_loss"] = torch.cat((total["frame_loss"], out["frame_loss"]))
                    total["reg"] = torch.cat((total["reg"], out["reg"]))
            return total
        total = None
        for c, (fp, cols) in enumerate(chans):
            if S_all is not None:
                S, s_ids = S_all[c], times
            else:
                S, s_ids = fp.recon_image(Cdev, times), None
            out = ops.warp_recon_grad(S, s_ids, frames if cols is None else frames[:, cols], frame_ids, fp.sz_list,
                                      fp.beta.detach(), times, grad=grad, want_loss=want, want_reg=want,
                                      workspace=self._ws_k2, norm_frames=norm * nc)
            self._ws_k2 = out["workspace"]
            if total is None:
                total = out
            elif want:
                total["loss"] += out["loss"]
                total["frame_loss"] += out["frame_loss"]
        return total

    def init_motion(self, P_T, order='quadratic', ridge=0.0):
        """Start the warp from tracks: ``fp.beta`` takes, in place, the ``beta`` that ``fp.beta_from_positions(P_T, order=order,
        ridge=ridge)`` fits to the positions ``P_T`` (K,3,T) (``MotionCorrect.apply_shifts_points``, the simulator, any
        tracker).  The leaf stays the same tensor object, so an optimiser built on ``[fp.beta]`` keeps working; ``.grad`` is
        cleared; frames the fit could not solve (``ok`` False) keep the coefficients they had.  Returns ``ok`` (T) bool.

        Call it before the first ``update_motion``: the optimiser's state (Adam's moments, its step count) is not touched,
        and moments gathered around another ``beta`` would pull the first steps the wrong way.  Nothing else needs
        resetting: every fit step reads ``fp.beta`` when it runs (the fused motion epoch coasts from the tensor itself, the
        reconstruction images depend on ``A`` and ``C`` only).  With the T axis sharded over ranks every rank passes the
        tracks of its own frames."""
        beta, ok = self.fp.beta_from_positions(P_T, order=order, ridge=ridge)
        if beta.shape != self.fp.beta.shape:
            raise ValueError(f"init_motion: tracks of {beta.shape[2]} frames for a model of {self.fp.beta.shape[2]}")
        with torch.no_grad():
            self.fp.beta.copy_(torch.where(ok[None, None, :], beta, self.fp.beta))
        self.fp.beta.grad = None
        return ok

    def track(self, frames, search=(6, 6, 1), predict=None, **kw):
        """The model's neurons followed through ``frames`` (what ``ExponentialFP.track_positions`` takes as ``video``) with
        the model's own centres ``fp.pos`` and width ``fp.sigma`` (K15): ``(P_T (K,3,T) float64, amplitudes (K,T))``, tracks
        that feed ``init_motion`` unchanged.  ``predict``: None looks around ``fp.pos`` in every frame, ``'model'`` around
        ``self.positions()`` -- tracking around the current warp -- and a (K,3,T) or (K,3) array around itself; ``kw``:
        ``threshold``, ``background``, ``exclude``.  Neighbouring neurons are not removed from the score, so a neuron within
        about 2 sigma of a brighter one can be captured by it: ``search`` is the guard, and ``exclude=R`` (K15x, R rounds) the
        remedy."""
        if isinstance(predict, str):
            if predict != 'model':
                raise ValueError(f"track: predict must be None, 'model' or positions, got {predict!r}")
            predict = self.positions()
        return ExponentialFP.track_positions(frames, self.fp.pos, shape_std=float(self.fp.sigma[0]), search=search, predict=predict, **kw)

    def follow(self, frames, anchor=0, start=None, search=(3, 3, 1), **kw):
        """The model's neurons followed through ``frames`` from the frame ``anchor``, forwards and backwards, each frame
        searched around what the frame before gave (K15c, ``ExponentialFP.follow_positions``, with the model's width
        ``fp.sigma``): ``(P_T (K,3,T) float64, amplitudes (K,T), info)``, also kept in ``self.last_follow``.  ``start`` (K,3):
        the centres in the anchor frame; None takes the model's centres there under the current warp,
        ``self.positions(times=[anchor])``.  ``kw``: ``momentum``, ``max_gap``, ``threshold``, ``background``.  Neurons are not
        excluded from one another: one within about 2 sigma of a brighter one can be captured by it."""
        if start is None:
            start = self.positions(times=[int(anchor)])[:, :, 0]
        self.last_follow = ExponentialFP.follow_positions(frames, start, shape_std=float(self.fp.sigma[0]), search=search, anchor=anchor, **kw)
        return self.last_follow

    def positions(self, points=None, times=None, start=None, tol=1e-6):
        """``fp.positions``: where the fitted warp puts the neurons in every frame, (K,3,T) float64 numpy."""
        return self.fp.positions(points=points, times=times, start=start, tol=tol)

    def update_motion(self, dataloader, optimizer, gamma=0, epochs=20, solver='adam', iters=None, damping=1e-3):
        """Reference :181-194: mini-batch steps of the caller's optimiser on ``fp.beta`` against
        ``mse(A_tC, frames) + gamma*mean(reg)`` (the reg term is gradient-free in the reference, :60-61).

        ``solver='gn'`` (not in the reference) fits every frame's warp by damped Gauss-Newton steps instead
        (``_update_motion_gn``: K16 + ``dnmf_lm_step``): no learning rate, ``optimizer`` may be None and is left untouched,
        ``iters`` (default ``epochs``) Levenberg-Marquardt iterations per frame starting at the damping ``damping``; ``gamma``
        is ignored, as the reference's gradient-free reg term is.  ``self.motion_smooth`` > 0 (``solver='gn'`` only; with any
        other solver, or negative or not finite, a ValueError) adds the temporal prior ``motion_smooth`` * sum_t |theta_t -
        theta_{t+1}|^2 to the mean squared error (K16s, see ``_update_motion_gn``): a frame whose neurons are dark is then
        carried by its neighbours in time instead of keeping its start.  ``self.motion_order`` (``solver='gn'`` only, checked the
        same way) chooses the coefficients that are fitted: ``'translation'``, ``'affine'``, ``'quadratic'`` (the default: all),
        ``'graded'`` -- the three in turn with ``iters`` iterations each, which reaches a warp several voxels away where the full
        order diverges -- or a sequence of ``(order, iterations)`` stages (K16o, see ``_update_motion_gn``).
        ``self.motion_jacobian`` > 0 (``solver='gn'`` only, checked the same way) adds the volume-preserving prior
        ``motion_jacobian`` * mean_p (log det J(u_p))^2 over the corners and the centre of the volume to the mean squared error
        (K16j, see ``_update_motion_gn``): a step to a map that folds at one of those points is never accepted.

        A ``ResidentLoader`` hands over rows that already live on the GPU.  Any other loader (the stock
        ``torch.utils.data.DataLoader`` of demo.py:33-35) is iterated once per epoch by a background thread while this
        thread copies the mini-batches into a device buffer (``_stage_epoch``); the epoch then runs from that buffer --
        as four launches when the optimiser is the demo's plain Adam (``_motion_epoch``), else step by step."""
        _check_motion_solver(solver, "update_motion")
        smooth = _check_motion_smooth(self.motion_smooth, solver, "update_motion")
        order = _check_motion_order(self.motion_order, solver, "update_motion")
        jacobian = _check_motion_jacobian(self.motion_jacobian, solver, "update_motion")
        if solver == 'gn':
            return self._update_motion_gn(dataloader, epochs if iters is None else iters, damping, gamma, smooth, order, jacobian)
        fp = self.fp
        beta = fp.beta
        # reconstruction images of all frames (C is constant inside this call): built when first needed -- the fused
        # epoch on compact footprints makes its own, chunk by chunk (_motion_epoch)
        cache = {}

        def recon():
            if not cache:
                cache["S"] = self._recon_cache()
                cache["C"] = None if cache["S"] is not None else self.C.to(device, torch.float32).contiguous()
            return cache["S"], cache["C"]

        chunked = self.motion_chunk > 0 and self._motion_lists_layout() is not None
        resident = isinstance(dataloader, ResidentLoader)
        for epoch in range(1, epochs + 1):
            if self.verbose:
                print('Epoch ' + str(epoch))
            fp.train()
            if resident:
                plan, frames, rows = dataloader.epoch_plan(), dataloader.frames_2d(), None
                norms = [min(dataloader.batch_size, dataloader.T_total - j * dataloader.batch_size)
                         for j in range(plan.nsteps)]
            else:
                staged = self._stage_epoch(dataloader) if self.stream_loader else None
                if staged is None:      # unknown length or too large to stage: batch by batch from the host
                    self._motion_epoch_from_host(dataloader, optimizer, *recon())
                    continue
                frames, batch_times, by_frame = staged
                plan = sharding.plan_from_batches(batch_times, fp.T)
                norms = [len(b) for b in batch_times]
                rows = None     # frame t in row t (a dataset's own device frames)
                if not by_frame:
                    # row of the staging buffer that holds frame t
                    flat = torch.tensor([t for b in batch_times for t in b], dtype=torch.int64)
                    rows = torch.zeros(fp.T, dtype=torch.int32)
                    rows[flat] = torch.arange(flat.numel(), dtype=torch.int32)
                    rows = rows.to(device)
                if plan is None:        # a frame served twice in one epoch: the steps as they come
                    plan = sharding.EpochPlan(len(batch_times), None, None, None, [torch.tensor(b, dtype=torch.int64)
                                                                                   for b in batch_times])
            if plan.frame_step is not None and self._fusable(optimizer) and (chunked or recon()[0] is not None):
                self._motion_epoch(plan, frames, rows, optimizer, None if chunked else recon()[0])
                continue
            S_all, Cdev = recon()
            for batch_idx, b in enumerate(plan.batches):
                optimizer.zero_grad()
                if beta.grad is None:
                    beta.grad = torch.zeros_like(beta)
                if b.numel() == 0:      # sharded: this global mini-batch has no frame here; still a step
                    optimizer.step()
                    continue
                times = b.to(device, torch.int32)
                want = self.verbose and batch_idx % 10 == 0
                out = self._k2(S_all, Cdev, frames, times if rows is None else rows[times.long()], times, beta.grad,
                               norms[batch_idx], want)
                optimizer.step()
                if want:
                    print('Recon: ' + str(out["loss"][0]))
                    print('Reg: ' + str(out["reg"]))

    def _update_motion_gn(self, dataloader, iters, damping, gamma=0, smooth=0.0, order='quadratic', jacobian=0.0):
        """``update_motion(solver='gn')``: Levenberg-Marquardt on the 30 (12 at Z = 1) coefficients of every frame.

        The loss is a sum over frames and frame t only sees ``beta[:, :, t]``, so the frames are independent small dense
        least-squares problems.  Chunk-outer, iteration-inner: for each chunk of frames the reconstruction images are built
        once (``fp.recon_image``: from the neuron lists when the footprints are compact; C is constant here), then ``iters``
        pairs of K16 (``ops.warp_normal_eqs``: H = J^T J, g = J^T r, sse at the trial coefficients, summed over the colour
        channels) and ``ops.lm_step`` (accept or reject the trial, next trial) run without a host synchronisation, and a last
        K16 + accept-only step leaves the best ACCEPTED coefficients in ``fp.beta`` -- never an untested trial.  The images of
        the whole video are never needed; a chunk is ``motion_chunk`` frames when that is set, else what fits
        ``GN_CHUNK_BYTES``.  A ``ResidentLoader`` and a stageable loader are served from their device rows in one pass (frame
        order is irrelevant); any other loader batch by batch, each mini-batch getting its iterations when it arrives.

        ``fp.beta`` is updated in place (``requires_grad`` kept, ``.grad`` left alone).  Afterwards ``last_motion_gn`` holds,
        per frame of the model (NaN / 0 for frames the loader did not serve), ``sse0`` and ``sse`` (squared error at the
        start and at the result), ``accepted`` / ``rejected`` step counts and the final damping ``lam``.  With the T axis
        sharded over ranks every rank fits its own frames: there is no collective and nothing to exchange.

        ``smooth`` (the model's ``motion_smooth``) > 0 (K16s, ``dnmf_lm_step_smooth``; tests/gn_smooth_restatement.py is the
        definition).  With theta_t the 30 (12) coefficients of frame t in K16's centred basis -- its monomials are O(1) over the
        volume, so theta is in voxels -- n the residuals of a frame (voxels x colour channels) and m = ``smooth`` n, the
        objective becomes
            F(beta) = sum_t sse_t + m sum_t |theta_t - theta_{t+1}|^2,
        F / n = mse + ``smooth`` * roughness: ``smooth`` is the mean squared error one is willing to pay per squared voxel of
        frame-to-frame change of a coefficient.  It is lowered by red-black block coordinate descent: ``beta_ref``, a copy of
        ``fp.beta`` made at entry, holds every frame's ACCEPTED coefficients; inside an iteration the chunk's frames of even t
        take K16 + step, then those of odd t, each reading its neighbours t +- 1 from ``beta_ref`` (never from ``fp.beta``,
        which holds untested trials between steps).  Same-colour frames do not interact, so every accepted step lowers F.
        The work per iteration is the same in twice the launches; a chunk's images are still built once.  A frame with
        H = 0 (dark neurons) takes a damped step to its neighbours' mean.  ``last_motion_gn`` gains ``prior``: per frame m
        sum_s |theta_t - theta_s|^2 of the result against its neighbours (NaN for frames not served); ``sse0`` / ``sse``
        stay the data term alone.
        * A chunk's boundary frames see what the neighbouring chunk currently holds in ``beta_ref`` -- its start values if
          that chunk comes later -- so ONE CALL carries information across a chunk boundary only once, and only forward;
          a mini-batch of a non-stageable loader is a chunk in this sense.  Call again (or raise ``motion_chunk``) when
          dark stretches span chunk boundaries.
        * With T sharded over ranks a shard's first and last frame treat the off-shard neighbour as absent; there is still
          no collective.
        * BIAS.  The prior is first order: it pulls a warp that moves linearly in time toward a constant one.  Float64
          definition, 7 frames, true warp linear in t, C[:, 3] = 0, identity start, 8 iterations, largest distance (voxels)
          between fitted and true warp per frame t = 0 .. 6:
              24x20x1  smooth 0     0      0      0      0.512  0      0      0
              24x20x1  smooth 1e-4  0.007  0.006  0.012  0.027  0.015  0.011  0.010
              24x20x2  smooth 0     0      0      0      0.402  0      0      0
              24x20x2  smooth 1e-4  0.017  0.013  0.017  0.030  0.028  0.024  0.023
          (0: below 5e-5).  At ``smooth`` = 1e-3 / 1e-2 every frame is 0.04 - 0.12 / 0.14 - 0.26 voxel off.

        ``order`` (the model's ``motion_order``; K16o, ``dnmf_lm_step_order``; tests/gn_order_restatement.py is the definition): a
        name, or stages ``((order, iterations), ...)`` run one after the other on each chunk -- ``'graded'`` is translation,
        affine, quadratic with ``iters`` iterations each.  A stage steps on the rows of the centred basis of its degree only (K16
        still returns the whole H and g; the step restricts them) and leaves the other rows of ``fp.beta`` bit for bit; it
        starts a fresh ``lm_state`` at the coefficients the stage before it accepted and ends with its own accept-only step.
        A chunk's images are still built once.  ``last_motion_gn`` gains ``stages``: a list with, per stage, dict(order, sse0,
        sse), per frame as above; the other keys describe the call: ``sse0`` from the first stage, ``sse`` / ``lam`` / ``prior``
        from the last, the counts summed.  ``'quadratic'``, the default, is the loop above, launch for launch, and its
        ``last_motion_gn`` has the keys it had: no ``stages``.

        ``jacobian`` (the model's ``motion_jacobian``) > 0 (K16j, ``dnmf_lm_step_jac``; tests/gn_jac_restatement.py is the
        definition): the paper's regulariser made to act.  With Jx the Jacobian of a frame's map in voxel coordinates -- the TRUE
        one, not the reference's ``log_det_jac`` with its xz / yz rows swapped -- at the sample points u_p
        (``ops.warp_jacobian_points``: the corners and the centre of the volume, 9 points, 5 at Z = 1), rho_p = log det Jx(u_p)
        (+inf where det Jx <= 0) and m_j = ``jacobian`` n, the objective becomes
            F(beta) = sum_t [sse_t + m_j mean_p rho_p^2],
        F / n = mse + ``jacobian`` * mean_p rho_p^2.  The step adds the term's exact Gauss-Newton Hessian and gradient on the
        unknowns of the stage's order; the accept test compares sse + temporal prior + this term, so a trial that folds at a
        sample point is never accepted after a frame's first call, and a start that folds is left at the first admissible
        trial.  det Jx is a cubic polynomial in u: nothing is claimed between the sample points.  No extra launches, no colours
        of its own; ``last_motion_gn`` gains ``jac`` (the term of the result) and ``min_det`` (its smallest det Jx over the
        sample points) per frame, NaN for frames not served.  0, the default, makes the calls and keeps the keys it had.
        * WHAT IT BUYS.  Float64 definition, K16o's problems (48 x 40 x Z, K = 6, T = 4, shift L), 16 full-order iterations from
          the identity, field error (voxels) / smallest det Jx, per weight 0 | 1e-4 | 1e-3 | 1e-2:
              Z 2 L 3 seed 0   1e-5 / 0.985  | 0.015 / 0.987  | 0.048 / 0.990 | 0.043 / 0.992
              Z 2 L 3 seed 1   19.1 / -5.7   | 0.047 / 0.983  | 0.031 / 0.984 | 0.057 / 0.986
              Z 2 L 3 seed 2   20.3 / -7.8   | 0.076 / 0.966  | 0.120 / 0.967 | 0.110 / 0.974
              Z 2 L 6 seed 0   81.9 / -31    | 8.8 / 0.076    | 7.0 / 0.81    | 16.1 / 0.79
              Z 2 L 6 seed 1   612 / -1430   | 20.6 / 0.060   | 41.8 / 0.010  | 48.9 / 0.55
              Z 2 L 6 seed 2   1390 / -121   | 16.2 / 0.14    | 0.069 / 0.966 | 0.26 / 0.90
              Z 1 L 3 seed 0   7e-6 / 0.980  | 0.0018 / 0.980 | 0.017 / 0.980 | 0.12 / 0.979
              Z 1 L 3 seed 1   2e-5 / 0.985  | 0.0028 / 0.985 | 0.023 / 0.985 | 0.10 / 0.988
              Z 1 L 3 seed 2   8e-6 / 0.974  | 0.0036 / 0.974 | 0.031 / 0.976 | 0.15 / 0.981
              Z 1 L 6 seed 0   73.4 / -0.26  | 52.6 / 0.037   | 68.1 / 0.44   | 38.8 / 0.74
              Z 1 L 6 seed 1   52.7 / 0.15   | 42.0 / 0.19    | 48.6 / 0.60   | 44.8 / 1.00
              Z 1 L 6 seed 2   8e-6 / 0.974  | 0.0099 / 0.974 | 0.069 / 0.975 | 0.21 / 0.980
          (a fit that leaves the basin is chaotic: its figure changes with the BLAS's rounding).  No cell with the prior ends
          folded; it rescues the two-slice fits 3 voxels away and one 6-voxel cell; ``'graded'`` stays the advice for far starts.
        * BIAS.  It pulls det Jx to 1.  Planted in-plane dilation by 1.03 on tests/gn_restatement.py's warps, 3 frames, 8
          iterations from the identity, largest distance (voxels) between fitted and true warp per frame:
              24x20x1  0     0       0       0             24x20x2  0     0       0       0
              24x20x1  1e-4  0.0004  0.0006  0.0011        24x20x2  1e-4  0.019   0.044   0.036
              24x20x1  1e-3  0.0042  0.0057  0.0102        24x20x2  1e-3  0.051   0.082   0.140
              24x20x1  1e-2  0.041   0.047   0.070         24x20x2  1e-2  0.065   0.137   0.164
          (0: below 5e-5).  Two slices say little about d q_z / d z, so there the prior moves that entry to buy det = 1."""
        fp = self.fp
        iters = int(iters)
        if iters < 0:
            raise ValueError(f"update_motion(solver='gn'): iters={iters}")
        schedule = [(o, iters) for o in MOTION_GRADED] if order == 'graded' else [(order, iters)] if isinstance(order, str) \
            else list(order)
        if self.verbose and gamma:
            print(f"update_motion(solver='gn'): gamma={gamma} ignored (the reg term is gradient-free in the reference)")
        chans = self._channels()
        row = sum(f.P for f, _ in chans)
        lds = ops.halo_voxels(fp.sz_list)
        chunk = int(self.motion_chunk) if self.motion_chunk > 0 else max(1, GN_CHUNK_BYTES // (4 * lds * len(chans)))
        chunk = min(chunk, K2_MAX_FRAMES)
        Cdev = self.C.to(device, torch.float32).contiguous()
        beta = fp.beta.detach()          # the same storage: the kernels read and write the leaf's columns
        stats = {"sse0": torch.full((fp.T,), float('nan'), dtype=torch.float64, device=device),
                 "sse": torch.full((fp.T,), float('nan'), dtype=torch.float64, device=device),
                 "accepted": torch.zeros((fp.T,), dtype=torch.int32, device=device),
                 "rejected": torch.zeros((fp.T,), dtype=torch.int32, device=device),
                 "lam": torch.full((fp.T,), float('nan'), dtype=torch.float64, device=device)}
        if order != 'quadratic':         # the default keeps the keys it had
            stats["stages"] = [{"order": o, "sse0": torch.full_like(stats["sse0"], float('nan')),
                                "sse": torch.full_like(stats["sse"], float('nan'))} for o, _ in schedule]
        beta_ref = None
        if smooth:
            stats["prior"] = torch.full((fp.T,), float('nan'), dtype=torch.float64, device=device)
            beta_ref = beta.clone()      # every frame's accepted coefficients: the neighbours a step reads
        step_kw = {}
        if jacobian:                     # the default keeps the keys and the call it had
            stats["jac"] = torch.full((fp.T,), float('nan'), dtype=torch.float64, device=device)
            stats["min_det"] = torch.full((fp.T,), float('nan'), dtype=torch.float64, device=device)
            step_kw["jacobian"] = jacobian
        bufs = {}

        def fit(frames, fid, times, host_times):
            """All iterations of the frames ``times`` (distinct; frame ``times[i]`` in row ``fid[i]``, None: row i);
            ``host_times``: the same list on the CPU (the colours are split there: no synchronisation)."""
            for s0 in range(0, times.numel(), chunk):
                tt = times[s0:s0 + chunk].contiguous()
                n = tt.numel()
                ff = None if fid is None else fid[s0:s0 + chunk].contiguous()
                fr = frames if fid is not None else frames[s0:s0 + n]
                if "S" not in bufs or bufs["S"][0].shape[0] < n:
                    bufs["S"] = [torch.empty((n, lds), dtype=torch.float32, device=device) for _ in chans]
                S = [f.recon_image(Cdev, tt, out=buf[:n]) for (f, _), buf in zip(chans, bufs["S"])]
                # colours: [rows of S, rows of fr, model times]; one colour of all frames without the prior, else the frames
                # of even t and those of odd t (each a launch of pairwise non-adjacent frames)
                colours = [(None, ff, tt)]
                if smooth:
                    colours = []
                    th = host_times[s0:s0 + chunk]
                    for parity in (0, 1):
                        pick = torch.nonzero(th % 2 == parity).reshape(-1)          # CPU
                        if pick.numel():
                            sel, pick = pick.to(device, torch.int32), pick.to(device)
                            colours.append((sel, sel if ff is None else ff[pick].contiguous(), tt[pick].contiguous()))
                for k, (stage_order, stage_iters) in enumerate(schedule):
                    # per colour its state and normal equations: every stage starts a fresh state at what is in beta
                    work = [[ops.lm_state(ct.numel(), device), None] for _, _, ct in colours]
                    for it in range(stage_iters + 1):
                        for (sel, cf, ct), w in zip(colours, work):
                            state, eqs = w
                            for c, ((f, cols), Sc) in enumerate(zip(chans, S)):
                                eqs = ops.warp_normal_eqs(Sc, sel, fr if cols is None else fr[:, cols], cf, fp.sz_list, beta, ct,
                                                          out=eqs, accumulate=c > 0, workspace=bufs.get("ws"))
                                bufs["ws"] = eqs["workspace"]
                            w[1] = eqs
                            ops.lm_step(state, eqs, fp.sz_list, beta, ct, lam0=damping, accept_only=it == stage_iters,
                                        smooth=smooth, n_residuals=row, beta_ref=beta_ref, order=stage_order, **step_kw)
                    for (_, _, ct), (state, _) in zip(colours, work):
                        idx = ct.long()
                        if "stages" in stats:
                            stats["stages"][k]["sse0"][idx], stats["stages"][k]["sse"][idx] = state["sse0"], state["sse"]
                        if k == 0:
                            stats["sse0"][idx], stats["accepted"][idx], stats["rejected"][idx] = state["sse0"], 0, 0
                        stats["sse"][idx], stats["lam"][idx] = state["sse"], state["lam"]
                        stats["accepted"][idx] += state["counts"][:, 0]
                        stats["rejected"][idx] += state["counts"][:, 1]
                        if smooth:
                            stats["prior"][idx] = state["prior"]
                        if jacobian:
                            stats["jac"][idx], stats["min_det"][idx] = state["jac"], state["min_det"]
                        if self.verbose:
                            print(f"GN frames {int(ct[0])}.. ({stage_order}): sse {float(state['sse0'].sum()):.6g} -> "
                                  f"{float(state['sse'].sum()):.6g}")

        with torch.no_grad():
            staged = None
            if isinstance(dataloader, ResidentLoader):
                staged = (dataloader.frames_2d(), [dataloader.order_tensor().tolist()], True)
            elif self.stream_loader:
                staged = self._stage_epoch(dataloader)
            if staged is not None:
                frames, batch_times, by_frame = staged
                flat = torch.tensor([t for b in batch_times for t in b], dtype=torch.int64)
                if frames.shape[1] != row:
                    raise ValueError(f"a frame has {frames.shape[1]} values, the model expects {row}")
                # frame t in row t, or in the (last) row of the staging buffer it arrived in
                rows = torch.zeros(fp.T, dtype=torch.int64)
                rows[flat] = flat if by_frame else torch.arange(flat.numel(), dtype=torch.int64)
                times = torch.unique(flat)
                fit(frames, rows[times].to(device, torch.int32), times.to(device, torch.int32), times)
            else:
                for data in dataloader:
                    times = torch.as_tensor(data[1]).to(device, torch.int32).reshape(-1)
                    fit(data[0].to(device, torch.float32).reshape(times.numel(), -1), None, times,
                        torch.as_tensor(data[1]).reshape(-1).to("cpu", torch.int64) if smooth else None)
        self.last_motion_gn = stats

    def _motion_epoch_from_host(self, dataloader, optimizer, S_all, Cdev):
        """One epoch with every mini-batch copied from the host when it is needed (loaders that cannot be staged)."""
        beta = self.fp.beta
        for batch_idx, data in enumerate(dataloader):
            times = torch.as_tensor(data[1]).to(device, torch.int32).reshape(-1)
            frames = data[0].to(device, torch.float32).reshape(times.numel(), -1)
            optimizer.zero_grad()
            if beta.grad is None:
                beta.grad = torch.zeros_like(beta)
            want = self.verbose and batch_idx % 10 == 0
            out = self._k2(S_all, Cdev, frames, None, times, beta.grad, 0, want)
            optimizer.step()
            if want:
                print('Recon: ' + str(out["loss"][0]))
                print('Reg: ' + str(out["reg"]))

    @staticmethod
    def _loader_frames(loader):
        """Frames one pass over ``loader`` yields, or None when that cannot be told without iterating it."""
        sampler = getattr(loader, "sampler", None)
        if getattr(loader, "dataset", None) is not None and sampler is not None and hasattr(sampler, "__len__") \
                and getattr(loader, "batch_size", None):
            n = len(sampler)
            return n // loader.batch_size * loader.batch_size if getattr(loader, "drop_last", False) else n
        if isinstance(loader, (list, tuple)):
            return sum(len(d[1]) for d in loader)
        return None

    def _stage_epoch(self, loader):
        """One pass over a host loader into a device buffer: returns ``(frames (n, row) fp32 CUDA rows in arrival
        order, [frame indices of every mini-batch])``, or None when the number of frames is unknown or the buffer would
        exceed ``STAGE_LIMIT``.  The loader is iterated by a background thread (its collate copies overlap the
        host-to-device copies issued here; pinned batches -- ``DataLoader(pin_memory=True)`` -- are copied
        asynchronously), and the buffer is kept between calls."""
        n = self._loader_frames(loader)
        row = sum(f.P for f, _ in self._channels())
        res = self._resident_batches(loader, row)
        if res is not None:
            return res[0], res[1], True
        if n is None or n == 0 or 4 * n * row > STAGE_LIMIT:
            return None
        if self._stage_buf is None or self._stage_buf.shape[0] < n or self._stage_buf.shape[1] != row:
            self._stage_buf = None
            self._stage_buf = torch.empty((n, row), dtype=torch.float32, device=device)
        buf = self._stage_buf
        batch_times, at = [], 0
        for data in _Prefetch(loader):
            idx = data[1].tolist() if hasattr(data[1], "tolist") else [int(i) for i in data[1]]
            if isinstance(idx, int):
                idx = [idx]
            B = len(idx)
            if at + B > n:
                raise RuntimeError(f"the loader yielded more than the {n} frames its length announces")
            src = data[0].reshape(B, -1)
            if src.shape[1] != row:
                raise ValueError(f"a frame has {src.shape[1]} values, the model expects {row}")
            buf[at:at + B].copy_(src, non_blocking=src.is_pinned() if hasattr(src, "is_pinned") else False)
            batch_times.append(idx)
            at += B
        return buf[:at], batch_times, False

    @staticmethod
    def _resident_batches(loader, row):
        """``(frames, index batches)`` of one pass over a stock single-process ``DataLoader`` whose dataset keeps its
        frames on the GPU (``dataset.device_frames()``: row t = frame t), without fetching a single sample: the
        loader's iterator is created as for an ordinary pass -- it draws the seeds an ordinary pass draws, so shuffled
        orders are the ones the reference loop would see -- and only its index batches are pulled.  None when the
        loader is anything else."""
        from torch.utils.data import DataLoader
        from torch.utils.data._utils.collate import default_collate
        from torch.utils.data.dataloader import _BaseDataLoaderIter
        if type(loader) is not DataLoader or loader.num_workers != 0 or loader.batch_sampler is None \
                or loader.collate_fn is not default_collate or not hasattr(_BaseDataLoaderIter, "_next_index"):
            return None
        get = getattr(loader.dataset, "device_frames", None)
        if get is None:
            return None
        frames = get()
        if frames.dim() != 2 or frames.shape[1] != row:
            return None
        it = iter(loader)
        batches = []
        while True:
            try:
                batches.append([int(i) for i in it._next_index()])
            except StopIteration:
                break
        return frames, batches

    def _fusable(self, optimizer):
        """True when ``optimizer`` is exactly the reference demo's: torch.optim.Adam([fp.beta]) without
        amsgrad / weight decay / maximize, so that its update can be evaluated per column in closed form."""
        if not self.fused_motion or type(optimizer) is not torch.optim.Adam or len(optimizer.param_groups) != 1:
            return False
        g = optimizer.param_groups[0]
        if len(g['params']) != 1 or g['params'][0] is not self.fp.beta:
            return False
        return not (g.get('amsgrad') or g.get('maximize') or g.get('weight_decay', 0) != 0 or g.get('capturable')
                    or g.get('differentiable') or g.get('fused') or g.get('decoupled_weight_decay'))

    def _motion_lists_layout(self):
        """The K3n layout when the motion gradient can take its reconstruction images from the neuron lists (one
        channel, compact footprints); else None."""
        if len(self._channels()) != 1 or not self.fp.use_lists:
            return None
        return self.fp.lists_layout()

    def _motion_epoch(self, plan, frames, rows, optimizer, S_all):
        """One epoch of mini-batch Adam steps: dnmf_adam_epoch phase 0, the gradient of every frame at its coasted
        beta, phase 1.  ``plan``: the epoch's EpochPlan; ``frames`` (n, row) device rows, frame t in row ``rows[t]``
        (``rows`` None: in row t).  ``S_all`` None: compact footprints, the reconstruction images are made
        ``motion_chunk`` frames at a time right before K2 gathers from them (``dnmf_motion_grad_lists``: they stay in
        the Infinity Cache); else the cached images of all frames and one K2 launch per group of equal mini-batch
        size.  The optimiser's own state tensors are read and written, so the caller's optimiser stays valid and a
        later un-fused step continues from it."""
        fp, beta = self.fp, self.fp.beta
        g = optimizer.param_groups[0]
        state = optimizer.state[beta]
        if len(state) == 0:  # what torch.optim.Adam._init_group creates on the first step()
            state['step'] = torch.tensor(0.0, dtype=torch.get_default_dtype())
            state['exp_avg'] = torch.zeros_like(beta, memory_format=torch.preserve_format)
            state['exp_avg_sq'] = torch.zeros_like(beta, memory_format=torch.preserve_format)
        n = plan.nsteps
        step0 = int(state['step'])
        args = (step0, plan.frame_step.to(device), n, g['lr'], g['betas'], g['eps'])
        order = plan.order.to(device)
        with torch.no_grad():
            ops.adam_epoch(beta, None, state['exp_avg'], state['exp_avg_sq'], *args, phase=0, order=order)
            grad = torch.zeros_like(beta)
            outs = []
            Cdev = self.C.to(device, torch.float32).contiguous() if S_all is None else None
            for idx, nf in plan.groups:
                if idx.numel() == 0:
                    continue
                idx = idx.to(device, torch.int32)
                fid = idx if rows is None else rows[idx.long()]
                if S_all is None:
                    out = ops.motion_grad_lists(self._motion_lists_layout(), fp.K, fp.sz_list, Cdev, frames, fid,
                                                beta.detach(), idx, grad, nf, self.motion_chunk, want=self.verbose,
                                                workspace=self._ws_mg)
                    self._ws_mg = out["workspace"]
                else:
                    out = self._k2(S_all, None, frames, fid, idx, grad, nf, self.verbose)
                outs.append((idx, nf, out))
            ops.adam_epoch(beta, grad, state['exp_avg'], state['exp_avg_sq'], *args, phase=1, order=order)
        state['step'] += n
        beta.grad = grad
        if self.verbose and outs:
            idx, nf, out = outs[0]
            for j in range(0, idx.numel() // nf, 10):
                print('Recon: ' + str(out["frame_loss"][j * nf:(j + 1) * nf].sum()))
                print('Reg: ' + str(out["reg"][j * nf:(j + 1) * nf]))

    def fit(self, dataloader, testloader, optimizer, batch_size, outer=5, gamma=1, epochs=10, gamma_c=0, iter_c=50,
            spatial=False, gamma_a=1e0, solver='mu', motion_solver='adam', registered='nearest', motion_smooth=None,
            background=0, background_rank=1, spatial_solver='mu', grow=0, iter_a=1, learn_colours=0, ar_g=None, ar_penalty=0.0,
            ar_baseline=0.0, motion_jacobian=None, motion_order=None):
        """Convenience wrapper of the loop ``demo.py:44-46`` writes out (not part of the reference).  ``spatial=True``
        also updates the footprints after every temporal update (``update_footprints(live_spatial=True)``); ``solver`` is
        that call's (``'hals'``: the exact trace solver K4h; ``'ar1'``: the AR(1)-constrained update K32, with its ``ar_g``,
        ``ar_penalty`` and ``ar_baseline`` and ``iter_c`` sweeps); ``motion_solver`` is ``update_motion``'s (``'gn'``: damped
        Gauss-Newton, ``optimizer`` may then be None) and ``motion_smooth`` the temporal prior's weight for the calls made
        here (``'gn'`` only; None: the model's ``motion_smooth``, 0 unless set; the attribute is put back afterwards);
        ``registered`` is ``update_footprints``' (``'linear'``: K17).  ``background=n > 0`` (K19): every sweep ends with
        ``update_background(testloader, iters=n)`` on the frames as given, and the following sweeps read
        ``background_loader(...)`` of both loaders, rebuilt after every background update; the first sweep sees the raw frames,
        because a background fitted before the model explains anything would take the neurons' mean light with it.  0: no
        background term, the path of a call without the argument.  ``background_rank=R``, 2 .. 8 (K23): those updates fit R
        images with R time courses (``update_background_rank``); 1: the rank-1 term.  ``motion_order`` is the model's
        ``motion_order`` for the calls made here, as ``motion_smooth`` is (``'gn'`` only; K16o, see ``update_motion``), and
        ``motion_jacobian`` the model's ``motion_jacobian`` in the same way (``'gn'`` only; K16j).
        ``spatial_solver``, ``grow`` and ``iter_a`` are ``update_footprints``' (``'hals'``: the exact footprint solver K6h,
        ``iter_a`` sweeps on supports grown by ``grow`` voxels; with ``verbose`` its max and median KKT are printed).
        ``learn_colours=n > 0`` (K29, ``MultiChannelDNMF`` only): every sweep ends with ``update_colours(testloader, sweeps=n)``
        on the frames the sweep's other steps read; 0: the colours stay, the path of a call without the argument."""
        _check_motion_solver(motion_solver, "fit")
        kept, kept_order, kept_jacobian = self.motion_smooth, self.motion_order, self.motion_jacobian
        motion_jacobian = _check_motion_jacobian(kept_jacobian if motion_jacobian is None else motion_jacobian, motion_solver, "fit")
        motion_smooth = _check_motion_smooth(kept if motion_smooth is None else motion_smooth, motion_solver, "fit")
        motion_order = kept_order if motion_order is None else motion_order
        _check_motion_order(motion_order, motion_solver, "fit")
        _check_registered(registered, "fit")
        if int(background) != background or background < 0:
            raise ValueError(f"fit: background is a number of alternations >= 0, got {background!r}")
        if int(background_rank) != background_rank or not 1 <= background_rank <= ops.BACKGROUND_RANKS[1]:
            raise ValueError(f"fit: background_rank={background_rank!r} (1 .. {ops.BACKGROUND_RANKS[1]})")
        if int(learn_colours) != learn_colours or learn_colours < 0:
            raise ValueError(f"fit: learn_colours is a number of sweeps >= 0, got {learn_colours!r}")
        if learn_colours and not hasattr(self, "update_colours"):
            raise ValueError("fit: learn_colours needs a MultiChannelDNMF (a single-channel model has no colours)")
        if background:
            self._background_refusals(dataloader, "fit(background=)")
            self._background_refusals(testloader, "fit(background=)")
        _check_trace_solver(solver)
        if solver == 'ar1':
            self._ar1_refusals(testloader, gamma_c)
        ar = dict(ar_g=ar_g, ar_penalty=ar_penalty, ar_baseline=ar_baseline) if solver == 'ar1' else {}
        out = (None, None, None)
        self.motion_smooth, self.motion_order, self.motion_jacobian = motion_smooth, motion_order, motion_jacobian
        try:
            train, test = dataloader, testloader
            for sweep in range(outer):
                self.update_motion(train, optimizer, gamma=gamma, epochs=epochs, solver=motion_solver)
                out = self.update_footprints(test, batch_size, self.fp.sz_list, gamma_c=gamma_c, gamma_a=gamma_a,
                                             iter_c=iter_c, live_spatial=spatial, solver=solver, registered=registered,
                                             spatial_solver=spatial_solver, grow=grow, iter_a=iter_a, **ar)
                if learn_colours:
                    self.update_colours(test, sweeps=int(learn_colours))
                if background:
                    if background_rank == 1:
                        self.update_background(testloader, iters=background)
                    else:
                        self.update_background_rank(testloader, iters=background, rank=background_rank)
                    if sweep + 1 < outer:
                        train = test = None      # the last sweep's cleaned frames go before the next ones are made
                        test = self.background_loader(testloader)
                        if dataloader is testloader:
                            train = test
                        elif isinstance(dataloader, ResidentLoader) and isinstance(testloader, ResidentLoader) \
                                and dataloader.frames_2d().data_ptr() == testloader.frames_2d().data_ptr() and dataloader.T == testloader.T:
                            # two loaders over one resident movie: one cleaned copy serves both
                            train = ResidentLoader(test.frames_2d(), self.fp.sz_list, dataloader.batch_size, shuffle=dataloader.shuffle,
                                                   generator=dataloader.generator)
                        else:
                            train = self.background_loader(dataloader)
        finally:
            self.motion_smooth, self.motion_order, self.motion_jacobian = kept, kept_order, kept_jacobian
        return out


class MultiChannelDNMF(DeformableNMF):
    """Several colour channels of one volume (BASELINE config 5, "C=3").  NOT in the reference, which has no channel
    axis on this path: the channels are treated as extra voxels that share the warp ``beta`` and the
    traces ``C`` -- channel ``c`` shows neuron ``k`` with footprint ``colours[c,k] * A[...,k]`` -- so every update
    formula of the reference holds with the sums over voxels also running over channels:
    ``G_t = sum_c A_t(c)^T A_t(c)``, ``r_t = sum_c A_t(c)^T y_t(c)``, loss = mean over batch x channels x voxels.

    A frame is the concatenation of its channels, ``(C, X, Y, Z)``: loaders yield ``(B, C, X, Y, Z)`` and a
    ``ResidentLoader`` is built on rows of ``C*P`` floats.  ``fp`` holds the uncoloured footprints and ``beta``."""

    def __init__(self, sz, K, T, colours, positions=None):
        super().__init__(sz, K, T, positions)
        colours = torch.as_tensor(colours, dtype=torch.float32).to(device)
        if colours.dim() != 2 or colours.shape[1] != K:
            raise ValueError(f"colours must be (channels, K={K}), got {tuple(colours.shape)}")
        self.colours = colours
        self._chan_fp = None
        self._chan_key = None
        # after update_colours: colours and kkt before / after, ok, ok_channel, scale, objective before / after of that call
        self.last_colours = None

    def _channels(self):
        import copy
        key = (self.fp.A.data_ptr(), self.fp.A._version, self.colours.data_ptr(), self.colours._version)
        if self._chan_fp is None or self._chan_key != key:
            P = self.fp.P
            self._chan_fp = []
            for c in range(self.colours.shape[0]):
                f = copy.copy(self.fp)  # shares beta (the caller's optimiser steps one tensor) and the lattice
                f.A = self.fp.A * self.colours[c]
                f.invalidate_layouts()   # a cache of its own: the copy shares the dict of self.fp
                self._chan_fp.append((f, slice(c * P, (c + 1) * P)))
            self._chan_key = key
        return self._chan_fp

    def _nchan(self):
        return self.colours.shape[0]

    def update_footprints(self, testloader, batch_size, sz, gamma_c=1e-2, gamma_a=1e0, iter_c=10, return_dense=False,
                          live_spatial=False, iter_a=1, solver='mu', registered='nearest', spatial_solver='mu', grow=0):
        """As DeformableNMF.update_footprints on the channel sums; the dense ``A_t`` return is not offered.  With
        ``live_spatial`` all channels are registered by one K7 call (one search per lattice point, a gather per channel;
        ``registered='linear'``: one K17 call, one solve per lattice point) and ``fp.A`` takes ``iter_a`` steps of
        ``spatial_step``."""
        if solver == 'ar1':
            raise ValueError("MultiChannelDNMF.update_footprints: solver='ar1' is a single-channel solver")
        if return_dense:
            raise NotImplementedError("MultiChannelDNMF.update_footprints: return_dense")
        return super().update_footprints(testloader, batch_size, sz, gamma_c=gamma_c, gamma_a=gamma_a, iter_c=iter_c,
                                         return_dense=False, live_spatial=live_spatial, iter_a=iter_a, solver=solver,
                                         spatial_solver=spatial_solver, grow=grow,
                                         registered=registered)

    def spatial_step(self, registered, D=None, gamma=None, frame_ids=None, times=None, solver='mu', sweeps=1, grow=0):
        """One multiplicative update of the (uncoloured) footprints ``fp.A`` from the registered frames of ALL channels
        (rows of NC * P floats).  With channel c showing neuron k as ``colours[c,k] A[:,k]`` the update of the shared ``A``
        that the reference's formula (``Demix/dNMF.py:151-160``) becomes is

            A <- A * (sum_c colours_c (Y_i^c C^T)) / (A (C C^T * colours^T colours) + gamma D + 1e-32)

        (numerator: K5 over the channels, weighted by their colours; denominator: K6 with C_s multiplied entry by entry by
        the Gram matrix of the colours).  The form is chosen as in DeformableNMF.spatial_step (``_spatial_lists``): the list
        form folds the colours into one channel K5 launch (``dnmf_spatial_accum_lists_channels``), the dense form runs K5
        per channel (by groups of 128 neurons beyond K = 128).  One all-reduce of the A1 | C_s buffer over ``self.group``
        like the single-channel step.  Not in the reference (no channel axis there): checked against this formula in
        float64 and, for one channel of colour 1, against ``DeformableNMF.spatial_step``.  ``solver='hals'``, ``sweeps``,
        ``grow``: the exact solver K6h on the same fused sums (see ``DeformableNMF.spatial_step``)."""
        NC, P = self.colours.shape[0], self.fp.P
        if registered.shape[1] != NC * P:
            raise ValueError(f"MultiChannelDNMF.spatial_step: rows of {registered.shape[1]} floats, expected {NC} x {P}")
        return super().spatial_step(registered, D=D, gamma=gamma, frame_ids=frame_ids, times=times, solver=solver, sweeps=sweeps,
                                    grow=grow)

    def _spatial_numerator(self, registered, C, sl, A1, Cs, frame_ids, times):
        fp = self.fp
        P, K = fp.P, fp.K
        if sl is not None:
            _, _, self._ws_k5 = ops.spatial_accum_lists_channels(registered, C, self.colours, sl, fp.sz_list, K, frame_ids=frame_ids,
                                                                 times=times, A1c=A1, Cs=Cs, workspace=self._ws_k5)
        else:
            A1.zero_()
            part = torch.empty((P, K), dtype=torch.float32, device=device)
            for c in range(self.colours.shape[0]):
                self._spatial_accum_dense(registered[:, c * P:(c + 1) * P], C, part, Cs, frame_ids, times)
                A1.addcmul_(part, self.colours[c][None, :])

    def _scale_Cs(self, Cs):
        Cs.mul_(self.colours.T @ self.colours)

    def update_colours(self, loader, sweeps=10, normalise=True, dry_run=False):
        """Learns ``self.colours`` from the frames ``loader`` serves, with ``fp.A``, ``fp.beta`` and ``self.C`` fixed (K29;
        tests/colours_restatement.py is the definition).  With A_t the UNCOLOURED warped footprints of frame t, G_t = A_t^T A_t
        and r_t^c = A_t^T y_t^c, the squared error of channel c is the quadratic 1/2 x^T M x - b_c^T x in x = colours[c, :],
        M[k, l] = sum_t G_t[k, l] C[k, t] C[l, t], b[c, k] = sum_t r_t^c[k] C[k, t]; each channel takes ``sweeps`` cyclic
        coordinate sweeps of the non-negative solver from its current colours (``ops.colour_normal_eqs``, ``ops.colour_solve``:
        float64).  ``sweeps`` is a parameter of the algorithm, not a tolerance; ``kkt`` in the result says how far from the
        solution the sweeps ended.  ``normalise``: colours[:, k] s with C[k, :] / s is the same model, so the largest colour of
        every neuron is then set to 1 and its trace rescaled.  A neuron whose trace is zero on these frames (M[k, k] = 0), or
        whose new colours are all zero or not finite, keeps its colours and its trace (``ok[k] = 0``): the step never kills a
        component.  A channel whose sums are not finite keeps its row (``ok_channel[c] = 0``).
        The frames go through in time order in pieces of at most 1 GiB; per piece and channel the Gram kernel that
        ``gram_kernel`` selects runs on the uncoloured ``fp`` (G is the same for every channel and is kept from the first).
        ``self.colours`` is replaced by a new tensor and ``self.C`` by a rescaled one; ``fp.A`` and its layouts stay.  Returns,
        and keeps in ``self.last_colours``, a dict of CUDA tensors: ``colours_before`` / ``colours`` (NC, K) fp32,
        ``kkt_before`` / ``kkt`` (NC) float64, ``ok`` (K) and ``ok_channel`` (NC) bool, ``scale`` (K) float64 the factor each
        trace was multiplied by, and the floats ``objective_before`` / ``objective`` = sum_c 1/2 x^T M x - b_c^T x, half the
        squared error up to a constant.  ``dry_run=True`` returns the same and leaves the model bit for bit as it was."""
        who = "update_colours"
        if self.group is not None or getattr(loader, "T_total", None) != getattr(loader, "T", None):
            raise NotImplementedError(f"{who}: the loader holds a shard of the frames (M and b would need an all-reduce)")
        fp = self.fp
        NC, K = self.colours.shape
        P = fp.P
        if NC > ops.COLOUR_MAX_NC or K > ops.COLOUR_MAX_K:
            raise ValueError(f"{who}: NC={NC} channels (<= {ops.COLOUR_MAX_NC}), K={K} neurons (<= {ops.COLOUR_MAX_K})")
        if int(sweeps) != sweeps or sweeps < 1:
            raise ValueError(f"{who}: sweeps={sweeps!r}, a whole number >= 1")
        with torch.no_grad():
            frames, order = self._frames_in_time_order(loader)
            if frames.dim() != 2 or frames.shape[1] != NC * P:
                raise ValueError(f"{who}: rows of {frames.shape[-1]} floats, expected {NC} x {P}")
            T = frames.shape[0]
            C = self.C.to(device, torch.float32)
            Cs = C[:, order.long()].contiguous()                     # the traces of the frames served, in time order
            step = _gib_rows(T, max(NC * P, K * K))
            nbr, state, M, b = self._gram_nbr, None, None, None
            for s in range(0, T, step):
                fr, tt = frames[s:s + step], order[s:s + step]
                G, rs = None, []
                for c in range(NC):
                    Gc, rc = self._gram_rhs_one(fp, fr[:, c * P:(c + 1) * P], tt)
                    if G is None:
                        G = Gc                                       # A_t^T A_t does not depend on the frames' values
                    rs.append(rc)
                    del Gc
                M, b, state = ops.colour_normal_eqs(G, torch.stack(rs), Cs[:, s:s + step], state=state, first=s == 0,
                                                    finish=s + step >= T)
            self._gram_nbr = nbr                                     # the pattern of the last COLOURED Gram matrices, for K4
            old = self.colours.contiguous()
            kkt0 = ops.colour_kkt(M, b, old)
            sol = ops.colour_solve(M, b, old, sweeps=int(sweeps))
            okc = sol["ok"] != 0
            new = sol["colours"].double()
            diag = torch.diagonal(M)
            top = new.max(0).values
            ok = torch.isfinite(new).all(0) & (top > 0) & torch.isfinite(diag) & (diag > 0)
            scale = torch.where(ok & bool(normalise), top, torch.ones_like(top))
            colours = torch.where(ok[None, :], new / scale[None, :], old.double()).float()

            def objective(x):
                x = x.double()
                return float((0.5 * torch.einsum("ck,kl,cl->c", x, M, x) - (b * x).sum(1)).sum())

            out = dict(colours_before=old, colours=colours, kkt_before=kkt0, kkt=sol["kkt"], ok=ok, ok_channel=okc, scale=scale,
                       objective_before=objective(old), objective=objective(sol["colours"]))
            if not dry_run:
                self.colours = colours
                self.C = (C.double() * scale[:, None]).float()
                self._chan_fp = None
                self.last_colours = out
        return out

    def _footprints_written(self):
        super()._footprints_written()
        self._chan_fp = None


def _mu_temporal(G, r, C, gamma, iters, group=None, nbr=None):
    """``iters`` multiplicative updates on (T,K,K) / (T,K) Gram data.

    ``C`` fp32 (K,T): the state update_footprints starts from (the reference's ``self.C``); without the
    neighbour term the whole loop is one K4 launch (fp64 inside, one rounding to fp32 at the end, as
    reference :177).  ``C`` fp64, or gamma != 0: the fp64 state is iterated with the one-round kernel.
    ``group``: torch.distributed group when the frames are a contiguous T-shard of rank order: with gamma != 0
    every round first exchanges the boundary columns (one all-gather of 2K doubles) so that the first / last frame
    of a shard sees its true neighbour instead of the replicated edge.  Returns a tensor of C's dtype."""
    if C.dtype == torch.float32 and (gamma is None or gamma == 0):
        return ops.mu_temporal(G, r, C.contiguous().clone(), iters, nbr=nbr)
    a = C.double().contiguous().clone()
    b = torch.empty_like(a)
    sharded = group is not None and gamma is not None and gamma != 0 and torch.distributed.get_world_size(group) > 1
    if sharded:
        rank, world = torch.distributed.get_rank(group), torch.distributed.get_world_size(group)
        edges = [torch.empty((2, a.shape[0]), dtype=torch.float64, device=a.device) for _ in range(world)]
    for _ in range(iters):
        left = right = None
        if sharded:
            mine = torch.stack((a[:, 0], a[:, -1])).contiguous()
            torch.distributed.all_gather(edges, mine, group=group)
            left = edges[rank - 1][1].contiguous() if rank > 0 else None
            right = edges[rank + 1][0].contiguous() if rank + 1 < world else None
        ops.mu_temporal_step(G, r, a, b, 0.0 if gamma is None else float(gamma), left, right)
        a, b = b, a
    return a.to(C.dtype)


SOLVERS = ('mu', 'hals')


def _check_solver(solver):
    if solver not in SOLVERS:
        raise ValueError(f"solver={solver!r}: expected one of {SOLVERS}")


TRACE_SOLVERS = SOLVERS + ('ar1',)   # update_footprints and fit: 'ar1' (K32) is a trace solver of the model only


def _check_trace_solver(solver):
    if solver not in TRACE_SOLVERS:
        raise ValueError(f"solver={solver!r}: expected one of {TRACE_SOLVERS}")


def _ar1_objective(G, r, C, g, penalty, baseline, chunk=256):
    """K32's objective F(C) = sum_t (1/2 c_t^T G_t c_t - r_t^T c_t) + sum_k penalty_k sum_t s_kt of a float64 state C (K, T) on
    the Gram data G (T, K, K), r (T, K), in float64, ``chunk`` frames at a time (tests/ar1_restatement.py: ``objective``)."""
    K, T = C.shape
    per = lambda v: torch.as_tensor(v, dtype=torch.float64).to(C.device).expand(K)   # noqa: E731
    f = torch.zeros((), dtype=torch.float64, device=C.device)
    for t0 in range(0, T, chunk):
        c = C[:, t0:t0 + chunk].t()                                   # (n, K)
        Gc = torch.einsum("tkl,tl->tk", G[t0:t0 + chunk].double(), c)
        f += (0.5 * (c * Gc).sum() - (r[t0:t0 + chunk].double() * c).sum())
    x = C - per(baseline)[:, None]
    s = x.clone()
    s[:, 1:] -= per(g)[:, None] * x[:, :-1]
    return float(f + (per(penalty) * s.sum(1)).sum())


def _check_spatial_solver(solver, sweeps, grow, who):
    """The footprint solver's arguments: 'mu' (K6) takes one update and no growth; 'hals' (K6h) ``sweeps`` >= 1 and
    ``grow`` >= 0 voxels, one number or (gx, gy, gz)."""
    _check_solver(solver)
    g = list(grow) if hasattr(grow, "__len__") else [grow] * 3
    if len(g) != 3 or any(int(v) != v or v < 0 for v in g):
        raise ValueError(f"{who}: grow={grow!r}, a whole number of voxels >= 0 or three of them")
    if int(sweeps) != sweeps or sweeps < 1:
        raise ValueError(f"{who}: sweeps={sweeps!r}, a whole number >= 1")
    if solver == 'mu' and (any(g) or sweeps != 1):
        raise ValueError(f"{who}: grow and sweeps belong to the 'hals' footprint solver (the multiplicative update keeps "
                         "every zero: it cannot use a grown support)")


def _check_registered(registered, who):
    if registered not in ('nearest', 'linear'):
        raise ValueError(f"{who}: registered must be 'nearest' (K7) or 'linear' (K17), got {registered!r}")


def _check_motion_solver(solver, who):
    if solver not in ('adam', 'gn'):
        raise ValueError(f"{who}: motion solver must be 'adam' or 'gn', got {solver!r}")


def _check_motion_smooth(smooth, solver, who):
    """The temporal prior's weight as a float: finite, >= 0, and non-zero only with the Gauss-Newton solver."""
    smooth = float(smooth)
    if not 0.0 <= smooth < float('inf'):
        raise ValueError(f"{who}: motion_smooth={smooth}: the temporal prior's weight must be finite and >= 0")
    if smooth and solver != 'gn':
        raise ValueError(f"{who}: motion_smooth={smooth} is supported by the motion solver 'gn' only (got {solver!r}); "
                         "Adam steps on the reference's loss, which has no temporal term")
    return smooth


def _check_motion_jacobian(jacobian, solver, who):
    """The volume-preserving prior's weight as a float: finite, >= 0, and non-zero only with the Gauss-Newton solver."""
    jacobian = float(jacobian)
    if not 0.0 <= jacobian < float('inf'):
        raise ValueError(f"{who}: motion_jacobian={jacobian}: the volume-preserving prior's weight must be finite and >= 0")
    if jacobian and solver != 'gn':
        raise ValueError(f"{who}: motion_jacobian={jacobian} is supported by the motion solver 'gn' only (got {solver!r}); "
                         "Adam steps on the reference's loss, whose reg term carries no gradient")
    return jacobian


MOTION_GRADED = ('translation', 'affine', 'quadratic')


def _check_motion_order(order, solver, who):
    """``motion_order`` as ``_update_motion_gn`` takes it: one of ``MOTION_GRADED`` or 'graded', or a tuple of (order,
    iterations) stages; anything but the default only with the Gauss-Newton solver."""
    if isinstance(order, str):
        if order != 'graded' and order not in MOTION_GRADED:
            raise ValueError(f"{who}: motion_order={order!r}: expected one of {MOTION_GRADED}, 'graded' or a sequence of "
                             "(order, iterations) stages")
    else:
        try:
            stages = tuple((o, int(n)) for o, n in order)
            if not stages or any(o not in MOTION_GRADED or n < 0 for o, n in stages) or any(int(n) != n for _, n in order):
                stages = ()
        except (TypeError, ValueError):
            stages = ()
        if not stages:
            raise ValueError(f"{who}: motion_order={order!r}: a schedule is a non-empty sequence of (order, iterations) with order "
                             f"one of {MOTION_GRADED} and iterations an int >= 0")
        order = stages
    if order != 'quadratic' and solver != 'gn':
        raise ValueError(f"{who}: motion_order={order!r} is supported by the motion solver 'gn' only (got {solver!r}); Adam steps "
                         "on all of beta")
    return order


def _hals_refuse_shards(gamma, group):
    """K4h's red-black order is defined on the whole time axis: the colour of a shard's first frame depends on its
    global offset and the edges need an exchange per half sweep.  Not built."""
    if gamma is not None and gamma != 0 and group is not None and torch.distributed.get_world_size(group) > 1:
        raise NotImplementedError("solver='hals' with gamma_c != 0 on a time axis sharded over ranks is not implemented: "
                                  "use solver='mu', gamma_c=0, or one rank")


def _hals_temporal(G, r, C, gamma, iters, group=None, nbr=None):
    """``iters`` sweeps of K4h on (T,K,K) / (T,K) Gram data, the counterpart of ``_mu_temporal``: ``(C', kkt)`` with C'
    of C's dtype and kkt (T) float64, the largest projected-gradient entry per frame after the last sweep.

    ``C`` fp32 and no neighbour term: one launch (fp64 inside, one rounding to fp32 at the end).  ``C`` fp64, or
    gamma != 0: an fp64 copy takes ``iters`` red-black sweeps of two launches each (even frames, then odd frames)."""
    _hals_refuse_shards(gamma, group)
    if C.dtype == torch.float32 and (gamma is None or gamma == 0):
        return ops.hals_temporal(G, r, C.contiguous().clone(), iters, nbr=nbr, kkt=True)
    a = C.double().contiguous().clone()
    g = 0.0 if gamma is None else float(gamma)
    for _ in range(iters):
        ops.hals_temporal_step(G, r, a, g, 0, nbr=nbr)
        ops.hals_temporal_step(G, r, a, g, 1, nbr=nbr)
    return a.to(C.dtype), ops.hals_temporal_kkt(G, r, a, g, nbr=nbr)


class _Prefetch:
    """Iterates ``loader`` in a background thread, two items ahead: the loader's own work (indexing the dataset,
    collating a mini-batch: host memory copies that release the GIL) overlaps what the consumer does with the
    previous item.  Exceptions of the loader are re-raised in the consumer."""

    _END = object()

    def __init__(self, loader, depth=2):
        import queue
        import threading
        self._q = queue.Queue(maxsize=depth)
        self._stop = False
        self._thread = threading.Thread(target=self._run, args=(loader,), daemon=True)
        self._thread.start()

    def _put(self, item):
        import queue
        while not self._stop:
            try:
                self._q.put(item, timeout=0.1)
                return
            except queue.Full:
                pass

    def _run(self, loader):
        try:
            for item in loader:
                self._put(item)
                if self._stop:
                    return
            self._put(self._END)
        except BaseException as exc:  # noqa: BLE001 - handed to the consumer
            self._put(exc)

    def __iter__(self):
        try:
            while True:
                item = self._q.get()
                if item is self._END:
                    return
                if isinstance(item, BaseException):
                    raise item
                yield item
        finally:
            self._stop = True


class ResidentLoader:
    """Iterates mini-batches of a video that already lives on the GPU as (T,P) rows.

    Yields ``(frames (B,X,Y,Z), idx int32 tensor)`` like a DataLoader over SimulatedVideoDataset; the fit steps
    recognise it and index the resident rows directly instead of copying batches (the timed region of bench.py
    starts with the inputs in HBM).  ``shuffle=True`` draws a new permutation per epoch from ``generator``.

    Sharded use (one process per GPU): ``frames`` holds the block ``[t0, t0+T_local)`` of a ``T_total``-frame
    video.  Every rank passes a generator with the SAME seed; mini-batches are cut from the global permutation
    and each rank keeps its own members (``dnmf_amd/sharding.py``), so the optimiser-step sequence is the
    single-process one."""

    def __init__(self, frames, sz, batch_size, shuffle=False, generator=None, t0=0, T_total=None):
        self.sz = _sz_list(sz)
        self._frames = frames.to(device, torch.float32).reshape(frames.shape[0], -1).contiguous()
        self.batch_size, self.shuffle, self.generator = int(batch_size), shuffle, generator
        self.T = self._frames.shape[0]
        self.t0 = int(t0)
        self.T_total = self.T if T_total is None else int(T_total)

    def frames_2d(self):
        return self._frames

    def order_tensor(self):
        return torch.arange(self.T, dtype=torch.int32, device=device)

    def __len__(self):
        return (self.T_total + self.batch_size - 1) // self.batch_size

    def epoch_plan(self):
        """Draw this epoch's (global) frame order and return its EpochPlan for the local block."""
        perm = torch.randperm(self.T_total, generator=self.generator) if self.shuffle else torch.arange(self.T_total)
        return sharding.plan_epoch(perm, self.batch_size, self.t0, self.t0 + self.T)

    def iter_indices(self):
        """Local frame indices of each (global) mini-batch, int32 on the GPU; empty for a mini-batch that has no
        frame in this block."""
        for b in self.epoch_plan().batches:
            yield b.to(device, torch.int32)

    def __iter__(self):
        for idx in self.iter_indices():
            yield self._frames[idx.long()].view(-1, *self.sz), idx


class SimulatedVideoDataset(Dataset):
    """Reference ``Demix/dNMF.py:196-217``: a synthetic video and its ground truth."""

    def __init__(self, K, T, sz, shape_std, density, bg_snr, traces, motion, motion_par, resident=False):
        """``resident=True`` (extension) renders the video on the GPU (``dnmf_render_frames``) and keeps it there,
        frame-major; ``video`` is then a CUDA view of shape (X,Y,Z,T) and ``loader()`` hands the rows to the fit
        steps without copies.  The noise is then drawn by the device generator, not the CPU one."""
        if resident:
            if traces != 'exp' or motion != 'gp':
                raise NotImplementedError("only traces='exp', motion='gp' are available")
            frames, positions, traces = Simulator.generate_video_resident(K, T, _sz_list(sz), shape_std, density, bg_snr,
                                                                          motion_par, device=device)
            video = frames.view(T, *_sz_list(sz)).permute(1, 2, 3, 0)
        else:
            video, positions, traces = Simulator.generate_video(K, T, _sz_list(sz), shape_std, density, bg_snr, traces,
                                                                motion, motion_par)
            # same values and the reference's (X,Y,Z,T) shape, but frame-major in memory: ``video[..., t]`` is then
            # one contiguous block instead of P floats that lie T apart (a cache line each)
            video = video.float().permute(3, 0, 1, 2).contiguous().permute(1, 2, 3, 0)
        self.video = video.float()
        self.positions = positions
        self.traces = traces
        self._sz = _sz_list(sz)

    def loader(self, batch_size, shuffle=False, generator=None):
        """A ResidentLoader over this video (clamped at 0 like ``__getitem__`` does frame by frame)."""
        frames = self.video.permute(3, 0, 1, 2).reshape(self.video.shape[3], -1)
        frames = frames.to(device).clamp_(min=0)
        return ResidentLoader(frames, self._sz, batch_size, shuffle=shuffle, generator=generator)

    def device_frames(self):
        """(T, P) fp32 rows on the GPU, row t = what ``self[t][0]`` returns (clamped at 0).  The fit steps take the
        frames of a stock ``DataLoader`` over this dataset from here instead of fetching and collating them one by one
        on the host (~80 us per 512x512 frame: 150 times the GPU work of a sweep); the stored video is clamped in place
        as a pass of ``__getitem__`` calls over all frames would leave it.  The copy is renewed when the stored
        video has been written to since."""
        v = self.video
        cached = getattr(self, "_device_frames", None)
        if cached is not None and cached[0] is v and cached[1] == v._version:
            return cached[2]
        v.clamp_(min=0)
        frames = v.permute(3, 0, 1, 2).reshape(v.shape[3], -1).to(device, torch.float32).contiguous()
        self._device_frames = (v, v._version, frames)
        return frames

    def __len__(self):
        return self.video.shape[3]

    def __getitem__(self, idx):
        if torch.is_tensor(idx):
            idx = idx.tolist()
        sample = self.video[:, :, :, idx]
        sample[sample < 0] = 0  # in place on the stored video, like the reference (:214-215)
        return sample, idx


class NeuroPALVideoDataset(Dataset):
    """Reference ``Demix/dNMF.py:220-248``: a recorded video (``data.mat``: ``data`` (X,Y,Z,T)) with tracked
    neuron positions (``traces_n.mat``: ``positions`` (K,3,T), 1-based; ``neuron_names``).  Same fixed
    sub-sampling as the reference (every 2nd voxel in x and y, every 10th in z, the first 100 frames); paths are
    joined portably (the reference hard-codes Windows separators).  The bodies of ``__init__`` and ``__getitem__`` restate
    reference ``Demix/dNMF.py:221-248`` almost line for line (``os.path.join`` instead of ``'\\'``): the file format, the
    sub-sampling and the rescaling of the positions are the interface, there is nothing to redesign in them."""

    def __init__(self, file):
        import os
        from scipy.io import loadmat
        vid_mat = loadmat(os.path.join(file, 'data.mat'))
        self.video = np.array(vid_mat['data'][::2, ::2, ::10, :100]).astype(np.float32)
        pos_mat = loadmat(os.path.join(file, 'traces_n.mat'))
        self.positions = torch.tensor(pos_mat['positions']).float() - 1
        self.positions[:, 0, :] /= 2
        self.positions[:, 1, :] /= 2
        self.positions[:, 2, :] /= 10
        self.names = pos_mat['neuron_names'][0]

    def device_frames(self):
        """(T, P) fp32 rows on the GPU, row t = what ``self[t][0]`` returns; see ``SimulatedVideoDataset.device_frames``.
        The video is a numpy array without a write counter, so the copy is made anew at every call (a pass over the
        100 frames the reference keeps)."""
        np.maximum(self.video, 0, out=self.video)
        T = self.video.shape[3]
        return torch.from_numpy(np.ascontiguousarray(np.moveaxis(self.video, 3, 0)).reshape(T, -1)).to(device, torch.float32)

    def __len__(self):
        return self.video.shape[3]

    def __getitem__(self, idx):
        if torch.is_tensor(idx):
            idx = idx.tolist()
        sample = self.video[:, :, :, idx]
        sample[sample < 0] = 0
        return sample, idx
